// Learned-aligner scores, the MFMA-free half (tacotron2_amd/alignment.py; the aligner of "One TTS Alignment
// To Rule Them All"): s(t,n) = z(t,n) - lse(t) + logp(t,n) with z = tau (2 q_t . k_n - |k_n|^2) from csrc/aligner.hip.
//   pack keys    Kp[n][c] = k[n][c] (zeros beyond C and at and beyond N_b), kn[n] = |k_n|^2 as an fmaf chain over c ascending.
//   transpose    out[c][r] = x[r][c] for r below the utterance's count, zeros up to the row's end: the B operands of the backward.
//   rows forward per frame t < T_b: m = max_n z, lse = m + log sum_n exp(z - m), s = (z - lse) + logp, in place; -inf at t >= T_b
//                and n >= N_b; lse kept where a backward follows.
//   rows backward per frame: G = sum_n g, p = exp(z - lse), dz = fmaf(-p, G, g) in place of z (zeros in the padding and in the
//                zero-fill up to Np), dlogp = g inside the utterance and 0 outside; then the column sums of dz.
//   prior        the beta-binomial log prior in float64 (lgamma), rounded once.
// A row belongs to one wave: lane l sums the columns l, l + 64, .. ascending, then the xor butterfly 32 .. 1 of t2_wave_sum,
// which gives every lane the same bits.  A column sum is four float64 partial sums over the frames j, j + 4, .., added as
// ((p0 + p1) + p2) + p3 and rounded once.  One writer per element, a fixed order, no atomics: two calls give the same bits and
// an utterance in a ragged batch gives the bits it gives alone.  Plain C++, __shfl_xor and __syncthreads only, so the CPU suite
// runs this very source on the host stand-in (tests/hip_emu).
#include "aligner.h"

__device__ __forceinline__ float al_ninf() { return __uint_as_float(0xff800000u); }

__device__ __forceinline__ float al_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// grid (ceil(N_max / 64), B), 256 lanes: 64 key rows a workgroup
__global__ void __launch_bounds__(256) aligner_pack_keys_kernel(const float* __restrict__ k, const int* __restrict__ n_len, int N_max,
                                                                int C, int Cp, float* __restrict__ Kp, float* __restrict__ kn) {
    const int b = blockIdx.y, n0 = blockIdx.x * 64, tid = threadIdx.x;
    const int N = t2_clamp_count(n_len[b], N_max);
    const float* kb = k + (long long)b * N_max * C;
    float* out = Kp + (long long)b * N_max * Cp;
    for (int i = tid; i < 64 * Cp; i += 256) {
        const int n = n0 + i / Cp, c = i % Cp;
        if (n < N_max) out[(long long)n * Cp + c] = (n < N && c < C) ? kb[(long long)n * C + c] : 0.0f;
    }
    if (tid < 64 && n0 + tid < N_max) {
        const int n = n0 + tid;
        float s = 0.0f;
        if (n < N)
            for (int c = 0; c < C; ++c) {
                const float v = kb[(long long)n * C + c];
                s = fmaf(v, v, s);
            }
        kn[(long long)b * N_max + n] = s;
    }
}

// grid (ceil(Rp / 256), C, B): out[b][c][r], r < Rp
__global__ void __launch_bounds__(256) aligner_transpose_kernel(const float* __restrict__ x, const int* __restrict__ lens, int R_max,
                                                                int C, int Rp, float* __restrict__ out) {
    const int b = blockIdx.z, c = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    const int R = t2_clamp_count(lens[b], R_max);
    if (r < Rp) out[((long long)b * C + c) * Rp + r] = r < R ? x[((long long)b * R_max + r) * C + c] : 0.0f;
}

// grid (ceil(T_max / AL_ROWS), B), 256 lanes; wave w takes the rows 4 i + w of the workgroup's sixteen
__global__ void __launch_bounds__(256) aligner_rows_fwd_kernel(float* __restrict__ scores, long long sb, long long st,
                                                               const float* __restrict__ logp, long long pb, long long pt,
                                                               const int* __restrict__ t_len, const int* __restrict__ n_len,
                                                               int T_max, int N_max, float* __restrict__ lse) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = t2_clamp_count(t_len[b], T_max), N = t2_clamp_count(n_len[b], N_max);
    const float ninf = al_ninf();
    for (int i = 0; i < AL_ROWS / 4; ++i) {
        const int t = blockIdx.x * AL_ROWS + 4 * i + wave;
        const bool row = t < T;                                             // uniform in the wave
        float* s = scores + b * sb + (long long)(t < T_max ? t : T_max - 1) * st;
        float m = ninf;
        if (row)
            for (int n = lane; n < N; n += 64) m = s[n] > m ? s[n] : m;
        m = al_wave_max(m);                                                 // every lane of the workgroup takes part
        float sum = 0.0f;
        if (row)
            for (int n = lane; n < N; n += 64) sum += expf(s[n] - m);
        sum = t2_wave_sum(sum);
        const float l = m + logf(sum);
        if (t < T_max) {
            const float* lp = logp ? logp + b * pb + (long long)t * pt : nullptr;
            for (int n = lane; n < N_max; n += 64) {
                float v = ninf;
                if (row && n < N) {
                    v = s[n] - l;
                    if (lp) v += lp[n];
                }
                s[n] = v;
            }
            if (lse && row && lane == 0) lse[(long long)b * T_max + t] = l;
        }
    }
}

// the same grid; dz holds z on entry
__global__ void __launch_bounds__(256) aligner_rows_bwd_kernel(const float* __restrict__ g, long long gb, long long gt,
                                                               const int* __restrict__ t_len, const int* __restrict__ n_len,
                                                               int T_max, int N_max, int Np, const float* __restrict__ lse,
                                                               float* __restrict__ dz, float* __restrict__ dlogp, long long db,
                                                               long long dt) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = t2_clamp_count(t_len[b], T_max), N = t2_clamp_count(n_len[b], N_max);
    for (int i = 0; i < AL_ROWS / 4; ++i) {
        const int t = blockIdx.x * AL_ROWS + 4 * i + wave;
        const bool row = t < T;
        const int tc = t < T_max ? t : T_max - 1;
        const float* gr = g + b * gb + (long long)tc * gt;
        float G = 0.0f;
        if (row)
            for (int n = lane; n < N; n += 64) G += gr[n];
        G = t2_wave_sum(G);
        if (t < T_max) {
            float* zr = dz + ((long long)b * T_max + t) * Np;
            const float l = row ? lse[(long long)b * T_max + t] : 0.0f;
            for (int n = lane; n < Np; n += 64) zr[n] = (row && n < N) ? fmaf(-expf(zr[n] - l), G, gr[n]) : 0.0f;
            if (dlogp) {
                float* dr = dlogp + b * db + (long long)t * dt;
                for (int n = lane; n < N_max; n += 64) dr[n] = (row && n < N) ? gr[n] : 0.0f;
            }
        }
    }
}

// grid (ceil(N_max / 64), B), 256 lanes: 64 columns, four partial sums each
__global__ void __launch_bounds__(256) aligner_colsum_kernel(const float* __restrict__ dz, const int* __restrict__ t_len,
                                                             const int* __restrict__ n_len, int T_max, int N_max, int Np,
                                                             float* __restrict__ colsum) {
    __shared__ double part[4][64];
    const int b = blockIdx.y, c = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int T = t2_clamp_count(t_len[b], T_max), N = t2_clamp_count(n_len[b], N_max);
    const int n = blockIdx.x * 64 + c;
    double s = 0.0;
    if (n < N)
        for (int t = j; t < T; t += 4) s += (double)dz[((long long)b * T_max + t) * Np + n];
    part[j][c] = s;
    __syncthreads();
    if (j == 0 && n < N_max) colsum[(long long)b * N_max + n] = n < N ? (float)(((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) : 0.0f;
}

// grid (ceil(T_max N_max / 256), B)
__global__ void __launch_bounds__(256) aligner_prior_kernel(const int* __restrict__ t_len, const int* __restrict__ n_len, int T_max,
                                                            int N_max, double omega, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T_max * N_max) return;
    const int t = (int)(i / N_max), n = (int)(i % N_max);
    const int T = t2_clamp_count(t_len[b], T_max), N = t2_clamp_count(n_len[b], N_max);
    float v = al_ninf();
    if (t < T && n < N) {
        const double a = omega * (t + 1), bb = omega * (T - t), m = N - 1;
        const double choose = lgamma(m + 1.0) - lgamma(n + 1.0) - lgamma(m - n + 1.0);
        const double top = lgamma(n + a) + lgamma(m - n + bb) - lgamma(m + a + bb);
        const double bot = lgamma(a) + lgamma(bb) - lgamma(a + bb);
        v = (float)(choose + top - bot);
    }
    out[(long long)b * T_max * N_max + i] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

extern "C" int t2amd_aligner_workspace(int B, int T_max, int N_max, int C, int which, long long* bytes) {
    T2_REQUIRE(bytes, "aligner_workspace: null operand");
    T2_PROPAGATE(al_check("aligner_workspace", B, T_max, N_max, C));
    T2_REQUIRE(which >= 0 && which <= 2, "aligner_workspace: which must be 0 (forward), 1 (forward, kept) or 2 (backward)");
    *bytes = which == 2 ? al_bwd_ws(B, T_max, N_max, C).bytes : al_fwd_ws(B, T_max, N_max, C, which).bytes;
    return T2AMD_OK;
}

extern "C" int t2amd_aligner_pack_keys_f32(const float* k, const int* n_len, int B, int N_max, int C, float* Kp, float* kn,
                                           void* stream) {
    T2_REQUIRE(k && n_len && Kp && kn, "aligner_pack_keys: null operand");
    T2_PROPAGATE(al_check("aligner_pack_keys", B, 1, N_max, C));
    T2_REQUIRE(t2_aligned16(Kp), "aligner_pack_keys: the key slab is not aligned to 16 bytes");
    T2_LAUNCH(aligner_pack_keys_kernel, dim3((unsigned)t2_cdiv(N_max, 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream, k, n_len,
              N_max, C, (int)t2_round_up(C, 32), Kp, kn);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_aligner_transpose_f32(const float* x, const int* lens, int B, int R_max, int C, float* out, void* stream) {
    T2_REQUIRE(x && lens && out, "aligner_transpose: null operand");
    T2_PROPAGATE(al_check("aligner_transpose", B, R_max, 1, C));
    T2_REQUIRE(t2_aligned16(out), "aligner_transpose: the slab is not aligned to 16 bytes");
    const int Rp = (int)t2_round_up(R_max, 32);
    T2_LAUNCH(aligner_transpose_kernel, dim3((unsigned)t2_cdiv(Rp, 256), (unsigned)C, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
              x, lens, R_max, C, Rp, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_aligner_rows_fwd_f32(float* scores, long long sb, long long st, const float* logp, long long pb, long long pt,
                                          const int* t_len, const int* n_len, int B, int T_max, int N_max, float* lse, void* stream) {
    T2_REQUIRE(scores && t_len && n_len, "aligner_rows_fwd: null operand");
    T2_PROPAGATE(al_check("aligner_rows_fwd", B, T_max, N_max, 1));
    T2_REQUIRE(t2_strides_cover(sb, st, B, T_max, N_max), "aligner_rows_fwd: score strides shorter than the matrix");
    T2_REQUIRE(!logp || t2_strides_cover(pb, pt, B, T_max, N_max), "aligner_rows_fwd: prior strides shorter than the matrix");
    const long long sbytes = t2_span_bytes(sb, st, B, T_max, N_max), pbytes = t2_span_bytes(pb, pt, B, T_max, N_max);
    T2_REQUIRE(!(logp && t2_overlap(scores, sbytes, logp, pbytes)) && !(lse && t2_overlap(scores, sbytes, lse, 4LL * B * T_max)),
               "aligner_rows_fwd: the scores must not overlap the prior or the kept lse");
    T2_LAUNCH(aligner_rows_fwd_kernel, dim3((unsigned)t2_cdiv(T_max, AL_ROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, scores,
              sb, st, logp, pb, pt, t_len, n_len, T_max, N_max, lse);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_aligner_rows_bwd_f32(const float* g, long long gb, long long gt, const int* t_len, const int* n_len, int B,
                                          int T_max, int N_max, const float* lse, float* dz, float* colsum, float* dlogp,
                                          long long db, long long dt, void* stream) {
    T2_REQUIRE(g && t_len && n_len && lse && dz && colsum, "aligner_rows_bwd: null operand");
    T2_PROPAGATE(al_check("aligner_rows_bwd", B, T_max, N_max, 1));
    T2_REQUIRE(t2_strides_cover(gb, gt, B, T_max, N_max), "aligner_rows_bwd: gradient strides shorter than the matrix");
    T2_REQUIRE(!dlogp || t2_strides_cover(db, dt, B, T_max, N_max), "aligner_rows_bwd: prior gradient strides shorter than the matrix");
    const int Np = (int)t2_round_up(N_max, 32);
    const long long gbytes = t2_span_bytes(gb, gt, B, T_max, N_max), dbytes = t2_span_bytes(db, dt, B, T_max, N_max);
    const long long zbytes = 4LL * B * T_max * Np;
    T2_REQUIRE(!t2_overlap(dz, zbytes, g, gbytes) && !t2_overlap(dz, zbytes, lse, 4LL * B * T_max) &&
                   !t2_overlap(colsum, 4LL * B * N_max, dz, zbytes) && !t2_overlap(colsum, 4LL * B * N_max, g, gbytes) &&
                   !(dlogp && (t2_overlap(dlogp, dbytes, g, gbytes) || t2_overlap(dlogp, dbytes, dz, zbytes) ||
                               t2_overlap(dlogp, dbytes, lse, 4LL * B * T_max) || t2_overlap(dlogp, dbytes, colsum, 4LL * B * N_max))),
               "aligner_rows_bwd: outputs must not overlap the inputs or each other");
    T2_LAUNCH(aligner_rows_bwd_kernel, dim3((unsigned)t2_cdiv(T_max, AL_ROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, gb,
              gt, t_len, n_len, T_max, N_max, Np, lse, dz, dlogp, db, dt);
    T2_LAUNCH(aligner_colsum_kernel, dim3((unsigned)t2_cdiv(N_max, 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream, dz, t_len,
              n_len, T_max, N_max, Np, colsum);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_beta_binomial_log_prior_f32(const int* t_len, const int* n_len, int B, int T_max, int N_max, double scaling,
                                                 float* out, void* stream) {
    T2_REQUIRE(t_len && n_len && out, "beta_binomial_log_prior: null operand");
    T2_PROPAGATE(al_check("beta_binomial_log_prior", B, T_max, N_max, 1));
    T2_REQUIRE(scaling > 0.0 && scaling <= 1e6, "beta_binomial_log_prior: the scaling must lie in (0, 1e6]");
    T2_LAUNCH(aligner_prior_kernel, dim3((unsigned)t2_cdiv((long long)T_max * N_max, 256), (unsigned)B), dim3(256), 0,
              (hipStream_t)stream, t_len, n_len, T_max, N_max, scaling, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
