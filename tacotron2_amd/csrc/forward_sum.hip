// Forward-sum alignment likelihood and its gradient (tacotron2_amd/alignment.py; the alignment loss of
// "One TTS Alignment To Rule Them All"): the dynamic programme of csrc/align.hip with logaddexp in place of max and a second
// sweep in the other direction.
//   admissible path: n(0) = 0, n(T-1) = N-1, n(t) - n(t-1) in {0, 1}; 1 <= N <= T.
//   alpha:  a(0,0) = l(0,0), a(0,n>0) = -inf, a(t,n) = l(t,n) + logaddexp(a(t-1,n), a(t-1,n-1));  log Z = a(T-1, N-1).
//   beta:   b(T-1,N-1) = 0, b(T-1,n<N-1) = -inf, b(t,n) = logaddexp(l(t+1,n) + b(t+1,n), l(t+1,n+1) + b(t+1,n+1)).
//   gamma:  g(t,n) = exp(a(t,n) + b(t,n) - log Z) = d log Z / d l(t,n);  soft durations d(n) = sum_t g(t,n).
//   logaddexp(x, y) = max + log1p(exp(min - max)), and -inf where the max is -inf: a score of -inf marks an impossible cell and
//   never makes a NaN.  An utterance without any possible path has log Z = -inf and zeros for g and d.
// Normalisation (the numerical point of section 19.3): plain float32 log values reach 10^4 and a + b - log Z cancels them.  So
// the rows a lane holds are kept relative to an offset, renewed on every row: the workgroup takes the maximum m of the row over
// the utterance's columns (0 where that is -inf), subtracts it from the row and adds it to a float64 offset (A for alpha, B for
// beta).  A row of alpha is stored with its maximum at 0, and its offset A_t (float64) beside it.  log Z = A + a(T-1,N-1) in
// float64, rounded for the caller; the beta kernel forms it again from the last kept row, rounds A_t + B - log Z to float32
// once, and g = exp((a + b) + that).  The soft durations are summed in float64 and rounded once.
// Layout: that of align_kernel.  One workgroup of FS_W lanes per utterance, lane l owns the C consecutive columns l C ..
// l C + C - 1 (C = 1 or 4) in registers.  A step publishes the one value the neighbour needs in an LDS double buffer
// edge[2][FS_W] (alpha: the last column to lane l + 1; beta: the first column to lane l - 1, which loads that column's score
// itself), as it stands before
// the row's maximum is known, together with the lane's own maximum; step t uses slot t & 1.  Two __syncthreads() per step:
// after the first sixteen lanes reduce sixteen lane maxima each, after the second every lane reads the sixteen and subtracts
// the maximum from its own columns and from the neighbour's value alike.  A maximum does not depend on the order it is taken
// in.  Memory is touched in bursts of FS_ROWS rows (loads before the steps, stores after them), so a step's barriers wait for
// LDS only; the loads are unconditional, with clamped indices.
// One writer per element, fixed order, no atomics: two calls give the same bits and an utterance in a ragged batch gives the
// bits it gives alone.  Plain C++ and __syncthreads only, so the CPU suite runs this very source on the host stand-in
// (tests/hip_emu).
#include "common.h"

#define FS_W 256                        /* lanes of the workgroup */
#define FS_MAX_T 4096                   /* frames at most */
#define FS_MAX_C 4                      /* columns of a lane at most: FS_W FS_MAX_C = 1024 tokens */
#define FS_ROWS 16                      /* rows loaded and stored at a time */

__device__ __forceinline__ float fs_ninf() { return __uint_as_float(0xff800000u); }

__device__ __forceinline__ float fs_logaddexp(float x, float y) {
    const float hi = x > y ? x : y, lo = x > y ? y : x;
    const float r = hi + log1pf(expf(lo - hi));                             // lo - hi <= 0, or NaN where both are -inf
    return hi == fs_ninf() ? hi : r;
}

// The maximum over the workgroup of what every lane has put into red[FS_W], in every lane (0 where it is -inf); two barriers,
// the first of which also publishes whatever else the lanes wrote before the call.  red2[16].
__device__ __forceinline__ float fs_block_max(const float* red, float* red2, int l) {
    __syncthreads();
    if (l < 16) {
        float m = red[16 * l];
#pragma unroll
        for (int k = 1; k < 16; ++k) m = red[16 * l + k] > m ? red[16 * l + k] : m;
        red2[l] = m;
    }
    __syncthreads();
    float m = red2[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) m = red2[k] > m ? red2[k] : m;
    return m == fs_ninf() ? 0.0f : m;
}

static long long fs_slab_bytes(int B, int T_max, int N_max) { return 4LL * B * T_max * t2_round_up(N_max, 4); }

template <int C>
__global__ void __launch_bounds__(FS_W) forward_sum_alpha_kernel(const float* __restrict__ scores, long long sb, long long st,
                                                                 const int* __restrict__ t_len, const int* __restrict__ n_len,
                                                                 int T_max, int N_max, float* __restrict__ log_z,
                                                                 float* __restrict__ slab_all, double* __restrict__ offs_all, int ld,
                                                                 unsigned long long* __restrict__ stamps) {
    __shared__ float edge[2][FS_W];
    __shared__ float red[FS_W];
    __shared__ float red2[16];
    const int b = blockIdx.x, l = threadIdx.x;
    const unsigned long long clk0 = wall_clock64();
    const int T = t2_clamp_count(t_len[b], T_max < FS_MAX_T ? T_max : FS_MAX_T);
    const int N = t2_clamp_count(n_len[b], N_max < C * FS_W ? N_max : C * FS_W);
    if (T < 1 || N < 1 || N > T) {                                          // uniform; the host refuses such lengths
        if (l == 0) {
            log_z[b] = 0.0f;
            stamps[2 * b] = 0;
        }
        return;
    }
    const float* x = scores + b * sb;
    float* slab = slab_all ? slab_all + (long long)b * T_max * ld : nullptr;
    double* offs = slab_all ? offs_all + (long long)b * T_max : nullptr;
    const float ninf = fs_ninf();
    const int n0 = l * C;

    float a[C];
    int oc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        oc[c] = n0 + c < N ? n0 + c : N - 1;
        a[c] = ninf;
    }
    if (l == 0) a[0] = x[0];
    double A = 0.0;
    // ---- rows t0 .. t0 + FS_ROWS - 1 are finished (and kept) in this burst; the scores it loads are those of the rows after them
    for (int t0 = 0; t0 < T; t0 += FS_ROWS) {
        float row[FS_ROWS][C], keep[FS_ROWS][C];
#pragma unroll
        for (int d = 0; d < FS_ROWS; ++d)
#pragma unroll
            for (int c = 0; c < C; ++c) row[d][c] = x[(t0 + d + 1 < T ? t0 + d + 1 : T - 1) * st + oc[c]];
        double mineA = 0.0;                                                 // lane d keeps the offset of row t0 + d
#pragma unroll
        for (int d = 0; d < FS_ROWS; ++d) {
            const int t = t0 + d;
            if (t < T) {                                                    // uniform
                float mine = ninf;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (n0 + c < N && a[c] > mine) mine = a[c];
                red[l] = mine;
                edge[t & 1][l] = a[C - 1];
                const float m = fs_block_max(red, red2, l);
                A += (double)m;
                if (l == d) mineA = A;
#pragma unroll
                for (int c = 0; c < C; ++c) keep[d][c] = a[c] = a[c] - m;
                if (t + 1 < T) {                                            // uniform
                    float adv = l > 0 ? edge[t & 1][l - 1] - m : ninf;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float stay = a[c];
                        a[c] = row[d][c] + fs_logaddexp(stay, adv);
                        adv = stay;
                    }
                }
            }
        }
        if (slab) {
            if (n0 < N) {
#pragma unroll
                for (int d = 0; d < FS_ROWS; ++d)
                    if (t0 + d < T) {
                        float* cell = slab + (long long)(t0 + d) * ld + n0;
                        if constexpr (C == 1) *cell = keep[d][0];
                        else t2_st4(cell, make_float4(keep[d][0], keep[d][1], keep[d][2], keep[d][3]));   // n0 + 3 < ld, 16-byte aligned
                    }
            }
            if (l < FS_ROWS && t0 + l < T) offs[t0 + l] = mineA;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (n0 + c == N - 1) {
            log_z[b] = (float)(A + (double)a[c]);
            stamps[2 * b] = wall_clock64() - clk0;
        }
}

template <int C>
__global__ void __launch_bounds__(FS_W) forward_sum_beta_kernel(const float* __restrict__ scores, long long sb, long long st,
                                                                const int* __restrict__ t_len, const int* __restrict__ n_len,
                                                                int T_max, int N_max, const float* __restrict__ log_z,
                                                                const float* __restrict__ scale, float* __restrict__ grad,
                                                                long long gb, long long gt, float* __restrict__ soft,
                                                                const float* __restrict__ slab_all,
                                                                const double* __restrict__ offs_all, int ld,
                                                                unsigned long long* __restrict__ stamps) {
    __shared__ float edge[2][FS_W];
    __shared__ float red[FS_W];
    __shared__ float red2[16];
    const int b = blockIdx.x, l = threadIdx.x;
    const unsigned long long clk0 = wall_clock64();
    const int T = t2_clamp_count(t_len[b], T_max < FS_MAX_T ? T_max : FS_MAX_T);
    const int N = t2_clamp_count(n_len[b], N_max < C * FS_W ? N_max : C * FS_W);
    float* g = grad + b * gb;
    float* sd = soft ? soft + (long long)b * N_max : nullptr;
    const float ninf = fs_ninf();
    const float lz = log_z[b];
    const bool none = T < 1 || N < 1 || N > T || lz == ninf;                // uniform: lengths the host refuses, or no possible path
    for (int t = none ? 0 : T; t < T_max; ++t)                              // the padding rows (every row where there is no path)
        for (int n = l; n < N_max; n += FS_W) g[t * gt + n] = 0.0f;
    if (none) {
        if (sd)
            for (int n = l; n < N_max; n += FS_W) sd[n] = 0.0f;
        if (l == 0) stamps[2 * b + 1] = 0;
        return;
    }
    const float* x = scores + b * sb;
    const float* slab = slab_all + (long long)b * T_max * ld;
    const double* offs = offs_all + (long long)b * T_max;
    const float sc = scale ? scale[b] : 1.0f;
    const int n0 = l * C;

    float bt[C];
    double dsum[C];
    int oc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        oc[c] = n0 + c < N ? n0 + c : N - 1;
        bt[c] = n0 + c == N - 1 ? 0.0f : ninf;
        dsum[c] = 0.0;
    }
    const int ocr = n0 + C < N ? n0 + C : N - 1;                            // the first column of lane l + 1
    const int na = n0 < N ? n0 : (N - 1) / C * C;                           // the slab columns this lane loads: its own, or the last owner's
    const double lzd = offs[T - 1] + (double)slab[(long long)(T - 1) * ld + N - 1];   // log Z before it was rounded
    double Bo = 0.0;
    // ---- rows t_hi, t_hi - 1, ... of a burst; bt is b(t, .) of the row in hand, columns at and beyond N hold -inf
    for (int t_hi = T - 1; t_hi >= 0; t_hi -= FS_ROWS) {
        float row[FS_ROWS][C], al[FS_ROWS][C], rr[FS_ROWS];
        double at[FS_ROWS];
#pragma unroll
        for (int d = 0; d < FS_ROWS; ++d) {
            const int t = t_hi - d > 0 ? t_hi - d : 0;
#pragma unroll
            for (int c = 0; c < C; ++c) row[d][c] = x[t * st + oc[c]];
            rr[d] = x[t * st + ocr];
            if constexpr (C == 1) al[d][0] = slab[(long long)t * ld + na];
            else {
                const float4 v = t2_ld4(slab + (long long)t * ld + na);
                al[d][0] = v.x, al[d][1] = v.y, al[d][2] = v.z, al[d][3] = v.w;
            }
            at[d] = offs[t];
        }
#pragma unroll
        for (int d = 0; d < FS_ROWS; ++d) {
            const int t = t_hi - d;
            if (t >= 0) {                                                   // uniform
                float mine = ninf, u[C];
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (bt[c] > mine) mine = bt[c];
                red[l] = mine;
                edge[t & 1][l] = bt[0];
                const float m = fs_block_max(red, red2, l);
                Bo += (double)m;
                const float off = (float)(at[d] + Bo - lzd);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const bool in = n0 + c < N;
                    bt[c] -= m;
                    const float gam = in ? expf((al[d][c] + bt[c]) + off) : 0.0f;
                    dsum[c] += (double)gam;
                    al[d][c] = in ? sc * gam : 0.0f;
                    u[c] = in ? row[d][c] + bt[c] : ninf;
                }
                if (t > 0) {                                                // uniform
                    const float nxt = l < FS_W - 1 ? rr[d] + (edge[t & 1][l + 1] - m) : ninf;
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        bt[c] = n0 + c < N ? fs_logaddexp(u[c], c + 1 < C ? u[c + 1 < C ? c + 1 : c] : nxt) : ninf;
                }
            }
        }
#pragma unroll
        for (int d = 0; d < FS_ROWS; ++d)
            if (t_hi - d >= 0) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (n0 + c < N_max) g[(t_hi - d) * gt + n0 + c] = al[d][c];
            }
    }
    if (sd) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (n0 + c < N_max) sd[n0 + c] = (float)dsum[c];
    }
    if (l == 0) stamps[2 * b + 1] = wall_clock64() - clk0;
}

static int fs_check(int B, int T_max, int N_max, char* msg) {
    const char* what = !(B >= 1 && B <= 1048576)     ? "1 to 2^20 utterances"
                       : !(T_max >= 1 && N_max >= 1) ? "at least 1 frame and 1 token"
                       : !(T_max <= FS_MAX_T)        ? "at most 4096 frames"
                       : !(N_max <= FS_MAX_C * FS_W) ? "at most 1024 tokens"
                                                     : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, 160, "forward_sum: %s: B %d frames %d tokens %d", what, B, T_max, N_max);
    return T2AMD_ERR_ARG;
}

// the workspace: [alpha rows, float32, B T_max ld][row offsets, float64, B T_max] (both only where kept), then two 64-bit
// clock counts an utterance
static long long fs_kept_bytes(int B, int T_max, int N_max) { return fs_slab_bytes(B, T_max, N_max) + 8LL * B * T_max; }

extern "C" int t2amd_forward_sum_workspace(int B, int T_max, int N_max, int keep, long long* bytes) {
    char msg[160];
    T2_REQUIRE(bytes, "forward_sum_workspace: null operand");
    if (fs_check(B, T_max, N_max, msg) != T2AMD_OK) T2_FAIL(msg);
    *bytes = (keep ? fs_kept_bytes(B, T_max, N_max) : 0) + 16LL * B;
    return T2AMD_OK;
}

extern "C" int t2amd_forward_sum_f32(const float* scores, long long sb, long long st, const int* t_len, const int* n_len, int B,
                                     int T_max, int N_max, float* log_z, int keep, unsigned char* ws, long long ws_bytes,
                                     void* stream) {
    char msg[160];
    T2_REQUIRE(scores && t_len && n_len && log_z && ws, "forward_sum: null operand");
    if (fs_check(B, T_max, N_max, msg) != T2AMD_OK) T2_FAIL(msg);
    T2_REQUIRE(t2_strides_cover(sb, st, B, T_max, N_max), "forward_sum: score strides shorter than the matrix");
    const long long kept = keep ? fs_kept_bytes(B, T_max, N_max) : 0;
    T2_REQUIRE(ws_bytes >= kept + 16LL * B, "forward_sum: the workspace is smaller than t2amd_forward_sum_workspace asks for");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0, "forward_sum: the workspace is not aligned to 16 bytes");
    const long long sbytes = t2_span_bytes(sb, st, B, T_max, N_max);
    T2_REQUIRE(!t2_overlap(ws, ws_bytes, scores, sbytes) && !t2_overlap(log_z, 4LL * B, scores, sbytes),
               "forward_sum: outputs and workspace must not overlap the scores");
    float* slab = keep ? reinterpret_cast<float*>(ws) : nullptr;
    double* offs = keep ? reinterpret_cast<double*>(ws + fs_slab_bytes(B, T_max, N_max)) : nullptr;
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(ws + kept);
    const int ld = (int)t2_round_up(N_max, 4);
    if (N_max <= FS_W)
        T2_LAUNCH(forward_sum_alpha_kernel<1>, dim3((unsigned)B), dim3(FS_W), 0, (hipStream_t)stream, scores, sb, st, t_len, n_len,
                  T_max, N_max, log_z, slab, offs, ld, stamps);
    else
        T2_LAUNCH(forward_sum_alpha_kernel<FS_MAX_C>, dim3((unsigned)B), dim3(FS_W), 0, (hipStream_t)stream, scores, sb, st, t_len,
                  n_len, T_max, N_max, log_z, slab, offs, ld, stamps);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_forward_sum_bwd_f32(const float* scores, long long sb, long long st, const int* t_len, const int* n_len, int B,
                                         int T_max, int N_max, const float* log_z, const float* scale, float* grad, long long gb,
                                         long long gt, float* soft, unsigned char* ws, long long ws_bytes, void* stream) {
    char msg[160];
    T2_REQUIRE(scores && t_len && n_len && log_z && grad && ws, "forward_sum_bwd: null operand");
    if (fs_check(B, T_max, N_max, msg) != T2AMD_OK) T2_FAIL(msg);
    T2_REQUIRE(t2_strides_cover(sb, st, B, T_max, N_max), "forward_sum_bwd: score strides shorter than the matrix");
    T2_REQUIRE(t2_strides_cover(gb, gt, B, T_max, N_max), "forward_sum_bwd: gradient strides shorter than the matrix");
    const long long kept = fs_kept_bytes(B, T_max, N_max);
    T2_REQUIRE(ws_bytes >= kept + 16LL * B, "forward_sum_bwd: the workspace is smaller than t2amd_forward_sum_workspace asks for");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0, "forward_sum_bwd: the workspace is not aligned to 16 bytes");
    const long long sbytes = t2_span_bytes(sb, st, B, T_max, N_max), gbytes = t2_span_bytes(gb, gt, B, T_max, N_max);
    T2_REQUIRE(!t2_overlap(grad, gbytes, scores, sbytes) && !t2_overlap(grad, gbytes, ws, ws_bytes) &&
                   !t2_overlap(grad, gbytes, log_z, 4LL * B) && !(scale && t2_overlap(grad, gbytes, scale, 4LL * B)) &&
                   !(soft && (t2_overlap(soft, 4LL * B * N_max, scores, sbytes) || t2_overlap(soft, 4LL * B * N_max, ws, ws_bytes) ||
                              t2_overlap(soft, 4LL * B * N_max, grad, gbytes))),
               "forward_sum_bwd: outputs must not overlap the inputs, the workspace or each other");
    const float* slab = reinterpret_cast<const float*>(ws);
    const double* offs = reinterpret_cast<const double*>(ws + fs_slab_bytes(B, T_max, N_max));
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(ws + kept);
    const int ld = (int)t2_round_up(N_max, 4);
    if (N_max <= FS_W)
        T2_LAUNCH(forward_sum_beta_kernel<1>, dim3((unsigned)B), dim3(FS_W), 0, (hipStream_t)stream, scores, sb, st, t_len, n_len,
                  T_max, N_max, log_z, scale, grad, gb, gt, soft, slab, offs, ld, stamps);
    else
        T2_LAUNCH(forward_sum_beta_kernel<FS_MAX_C>, dim3((unsigned)B), dim3(FS_W), 0, (hipStream_t)stream, scores, sb, st, t_len,
                  n_len, T_max, N_max, log_z, scale, grad, gb, gt, soft, slab, offs, ld, stamps);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
