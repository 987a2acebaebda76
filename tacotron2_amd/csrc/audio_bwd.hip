// Mel front end, the way back (tacotron2_amd/audio.py TacotronSTFT.mel_spectrogram with a grad_fn, MelLoss).  The forward is
//   padded = reflect(y); spec = frames . FB^T; mag = sqrt(re^2 + im^2); mel = mag . MB^T; out = log(max(mel, clip)) transposed.
// The two products of the backward run on the GEMM of gemm.hip (d_mag = d_mel . MB, d_frames = d_spec . FB); this file holds
// the row passes between them and the loss on top, one launch each:
//   mel_log_bwd:        d_mel[r][m] = d_out[b][m][j] / mel[r][m] where mel >= clip (torch's clamp(min=) rule: the gradient
//                       passes at equality), exactly 0 elsewhere; the transpose back to frame rows goes through an LDS tile.
//   stft_magnitude_bwd: d_re = d_mag re / mag, d_im = d_mag im / mag with mag recomputed by magnitude_kernel's operations in
//                       their order (t2_power of common.h: the forward's bits); both exactly 0 where mag == 0 (a definition:
//                       sqrt has no derivative there and torch gives NaN).  The d_spec row is t2_dspec_store's.
//   stft_frames_fold:   overlap-add of the frame gradients and the fold of the reflect padding in one gather: sample t sums, in
//                       ascending padded position and ascending frame order, every frame entry that covers pad - t, pad + t
//                       and pad + 2 (T - 1) - t, each position taken when t2_reflect maps it onto t.  No d_padded buffer.
//   mel_l1_fwd / _bwd:  masked mean |out - target| as per-workgroup partial slots (t2amd_wg_partial_sum_f32 adds them in
//                       order) and sign(out - target) g / count inside the mask, exactly 0 outside.
// No atomics anywhere: every output element has one writer and every sum a fixed order, so two calls give the same bits.
// An output whose byte range meets an input's is refused (t2_overlap), not only one that starts where an input starts.
// No MFMA and no LDS-DMA here, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
//
// Access widths.  Rows whose stride is a multiple of 4 floats are read and written 16 bytes per lane: mel rows (n_mel = 80),
// d_mag rows (Fpad), d_frames rows (L), d_y.  A spec row has 2F = L + 2 floats (1026): its start alternates between 16- and
// 8-byte alignment and its imaginary half starts at an odd float, so stft_magnitude_bwd takes one bin per lane with 4-byte
// accesses, every wave instruction one contiguous 256-byte run, on all four of its streams.
#include "common.h"

#define AB_TJ 64                        /* frames per mel_log_bwd tile */
#define AB_TM 16                        /* mel channels per mel_log_bwd tile */

// ---- log-compress ------------------------------------------------------------------------------------------------------
// A workgroup owns AB_TJ frames x AB_TM channels of utterance b: reads d_out along the frames (its fast index), writes d_mel
// along the channels (its fast index).
__global__ void __launch_bounds__(256) mel_log_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ mel,
                                                          long long ld, float* __restrict__ d_mel, long long ldd, int n,
                                                          int n_mel, float clip, int vec) {
    __shared__ float tile[AB_TM][AB_TJ + 1];
    const int b = blockIdx.z, m0 = blockIdx.y * AB_TM, j0 = blockIdx.x * AB_TJ;
    const int tid = threadIdx.x;
    {
        const int jj = tid & (AB_TJ - 1), j = j0 + jj;
#pragma unroll
        for (int p = 0; p < AB_TM / 4; ++p) {
            const int mm = (tid >> 6) + 4 * p, m = m0 + mm;
            tile[mm][jj] = (m < n_mel && j < n) ? d_out[((long long)b * n_mel + m) * n + j] : 0.0f;
        }
    }
    __syncthreads();
    const int jj = tid >> 2, q = tid & 3, j = j0 + jj, m = m0 + 4 * q;
    if (j < n && m < n_mel) {
        const long long r = (long long)b * n + j;
        if (vec && m + 3 < n_mel) {
            const float4 v = t2_ld4(mel + r * ld + m);
            float4 o;
            o.x = v.x >= clip ? tile[4 * q + 0][jj] / v.x : 0.0f;
            o.y = v.y >= clip ? tile[4 * q + 1][jj] / v.y : 0.0f;
            o.z = v.z >= clip ? tile[4 * q + 2][jj] / v.z : 0.0f;
            o.w = v.w >= clip ? tile[4 * q + 3][jj] / v.w : 0.0f;
            t2_st4(d_mel + r * ldd + m, o);
        } else {
            for (int e = 0; e < 4 && m + e < n_mel; ++e) {
                const float v = mel[r * ld + m + e];
                d_mel[r * ldd + m + e] = v >= clip ? tile[4 * q + e][jj] / v : 0.0f;
            }
        }
    }
}

extern "C" int t2amd_mel_log_bwd_f32(const float* d_out, const float* mel, long long ld, float* d_mel, long long ldd, int B,
                                     int n, int n_mel, float clip, void* stream) {
    T2_REQUIRE(d_out && mel && d_mel, "mel_log_bwd: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && n > 0 && n_mel > 0 && n_mel <= 65535 * AB_TM && ld >= n_mel && ldd >= n_mel,
               "mel_log_bwd: bad dims");
    T2_REQUIRE((long long)B * n <= T2_MAX_ROWS, "mel_log_bwd: at most 2^31 - 256 frame rows");
    T2_REQUIRE(clip > 0.0f, "mel_log_bwd: clip must be positive");
    const long long R = (long long)B * n, d_bytes = ((R - 1) * ldd + n_mel) * 4;
    T2_REQUIRE(!t2_overlap(d_mel, d_bytes, mel, ((R - 1) * ld + n_mel) * 4) && !t2_overlap(d_mel, d_bytes, d_out, R * n_mel * 4),
               "mel_log_bwd: d_mel must not be one of the inputs");
    const int vec = ld % 4 == 0 && ldd % 4 == 0 && t2_aligned16(mel) && t2_aligned16(d_mel);
    dim3 grid(t2_cdiv(n, AB_TJ), t2_cdiv(n_mel, AB_TM), B);
    T2_LAUNCH(mel_log_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_out, mel, ld, d_mel, ldd, n, n_mel, clip, vec);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- magnitude ---------------------------------------------------------------------------------------------------------
// Lane = bin f of row r; the row of d_spec is t2_dspec_store's (common.h).
__global__ void __launch_bounds__(256) magnitude_bwd_kernel(const float* __restrict__ d_mag, long long ldm,
                                                            const float* __restrict__ spec, long long lds,
                                                            float* __restrict__ d_spec, long long ldd, long long rows, int F,
                                                            int Kp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * F) return;
    const long long r = i / F;
    const int f = (int)(i - r * F);
    const float re = spec[r * lds + f], im = spec[r * lds + F + f];
    const float mag = sqrtf(t2_power(re, im));                          // magnitude_kernel's own arithmetic
    float dre = 0.0f, dim = 0.0f;
    if (mag != 0.0f) {
        const float g = d_mag[r * ldm + f] / mag;
        dre = __fmul_rn(g, re);
        dim = __fmul_rn(g, im);
    }
    t2_dspec_store(d_spec, r * ldd, f, F, Kp, dre, dim);
}

extern "C" int t2amd_stft_magnitude_bwd_f32(const float* d_mag, long long ldm, const float* spec, long long lds, float* d_spec,
                                            long long ldd, long long rows, int F, int Kp, void* stream) {
    T2_REQUIRE(d_mag && spec && d_spec, "stft_magnitude_bwd: null operand");
    T2_REQUIRE(rows > 0 && rows <= T2_MAX_ROWS && F > 0 && F <= 65536, "stft_magnitude_bwd: bad dims (at most 2^31 - 256 rows)");
    T2_REQUIRE(ldm >= F && lds >= 2 * (long long)F, "stft_magnitude_bwd: row too short");
    unsigned blocks;
    T2_PROPAGATE(t2_dspec_blocks("stft_magnitude_bwd", rows, F, Kp, ldd, &blocks));
    const long long d_bytes = ((rows - 1) * ldd + Kp) * 4;
    T2_REQUIRE(!t2_overlap(d_spec, d_bytes, spec, ((rows - 1) * lds + 2 * (long long)F) * 4) &&
                   !t2_overlap(d_spec, d_bytes, d_mag, ((rows - 1) * ldm + F) * 4),
               "stft_magnitude_bwd: d_spec must not be one of the inputs");
    T2_LAUNCH(magnitude_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_mag, ldm, spec, lds, d_spec, ldd, rows, F, Kp);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- overlap-add + reflect fold ------------------------------------------------------------------------------------------
// Frame j of an utterance covers padded positions [j hop, j hop + L), j < n; acc takes the frames that cover q in ascending j.
__device__ __forceinline__ void ab_cover_add(float& acc, const float* __restrict__ rows, long long ldf, long long q, int n,
                                             int L, int hop) {
    long long j1 = q / hop, j0 = (q - L + hop) / hop;
    if (q - L + 1 <= 0) j0 = 0;
    if (j1 > n - 1) j1 = n - 1;
    for (long long j = j0; j <= j1; ++j) acc += rows[j * ldf + (q - j * hop)];
}

// a padded position q other than pad + t that the pad maps onto sample t
__device__ __forceinline__ bool ab_mirror_of(long long q, long long t, int T, int pad) {
    return q >= 0 && q < (long long)T + 2 * pad && q != pad + t && t2_reflect(q - pad, T) == t;
}

// Thread = 4 consecutive samples of utterance blockIdx.y.  vec: pad, hop, L and ldf are multiples of 4 and d_frames is 16-byte
// aligned, so the four direct positions share their covering frames and each frame gives them one 16-byte load.
__global__ void __launch_bounds__(256) frames_fold_kernel(const float* __restrict__ d_frames, long long ldf,
                                                          float* __restrict__ d_y, long long ldy, int T, int n, int L, int hop,
                                                          int pad, int vec, int vec_out) {
    const int b = blockIdx.y;
    const long long t0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (t0 >= T) return;
    const float* rows = d_frames + (long long)b * n * ldf;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                       // left mirror: pad - t, 1 <= t <= pad
        const long long t = t0 + e, q = pad - t;
        if (t < T && ab_mirror_of(q, t, T, pad)) ab_cover_add(acc[e], rows, ldf, q, n, L, hop);
    }
    if (vec && t0 + 3 < T) {                                            // the sample's own position pad + t
        const long long q = pad + t0;
        long long j1 = q / hop, j0 = (q - L + hop) / hop;
        if (q - L + 1 <= 0) j0 = 0;
        if (j1 > n - 1) j1 = n - 1;
        for (long long j = j0; j <= j1; ++j) {
            const float4 v = t2_ld4(rows + j * ldf + (q - j * hop));
            acc[0] += v.x;
            acc[1] += v.y;
            acc[2] += v.z;
            acc[3] += v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t0 + e < T) ab_cover_add(acc[e], rows, ldf, pad + t0 + e, n, L, hop);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                       // right mirror: pad + 2 (T - 1) - t, T - 1 - pad <= t <= T - 2
        const long long t = t0 + e, q = (long long)pad + 2 * ((long long)T - 1) - t;
        if (t < T && ab_mirror_of(q, t, T, pad)) ab_cover_add(acc[e], rows, ldf, q, n, L, hop);
    }
    float* o = d_y + b * ldy + t0;
    if (vec_out && t0 + 3 < T) {
        t2_st4(o, make_float4(acc[0], acc[1], acc[2], acc[3]));
    } else {
        for (int e = 0; e < 4 && t0 + e < T; ++e) o[e] = acc[e];
    }
}

extern "C" int t2amd_stft_frames_fold_f32(const float* d_frames, long long ldf, long long f_floats, float* d_y, long long ldy,
                                          long long y_floats, int B, int T, int n, int L, int hop, int pad, void* stream) {
    T2_REQUIRE(d_frames && d_y, "stft_frames_fold: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && T > 0 && L > 0 && hop > 0 && hop <= L && pad >= 0, "stft_frames_fold: bad dims");
    T2_REQUIRE(pad < T, "stft_frames_fold: padding must be smaller than the signal (torch reflect rule)");
    T2_REQUIRE(n == T / hop + 1, "stft_frames_fold: n must be T / hop + 1 frames");
    T2_REQUIRE((long long)(n - 1) * hop + L <= (long long)T + 2 * pad, "stft_frames_fold: the frames reach beyond the padded signal");
    T2_REQUIRE((long long)B * n <= T2_MAX_ROWS, "stft_frames_fold: at most 2^31 - 256 frame rows");
    T2_REQUIRE(ldf >= L && f_floats >= ((long long)B * n - 1) * ldf + L, "stft_frames_fold: d_frames is shorter than its B n rows of L");
    T2_REQUIRE(ldy >= T && y_floats >= ((long long)B - 1) * ldy + T, "stft_frames_fold: d_y is shorter than (B, T)");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(d_frames) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_y) & 3u) == 0,
               "stft_frames_fold: operands misaligned");
    const int vec = pad % 4 == 0 && hop % 4 == 0 && L % 4 == 0 && ldf % 4 == 0 && t2_aligned16(d_frames);
    const int vec_out = ldy % 4 == 0 && t2_aligned16(d_y);
    dim3 grid(t2_cdiv(t2_cdiv(T, 4), 256), B);
    T2_LAUNCH(frames_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_frames, ldf, d_y, ldy, T, n, L, hop, pad, vec, vec_out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- masked L1 loss ------------------------------------------------------------------------------------------------------
// out (B, n_mel, n), target (B, n_mel, N), N <= n; utterance b counts its first lens[b] frames (lens NULL: N).  A workgroup
// owns `rpb` consecutive (b, m) rows: a thread adds its frames in ascending order in float64, the wave butterfly and the four
// wave sums follow in a fixed order, and the workgroup stores sum / count as its partial slot.
__device__ __forceinline__ int ab_len(const int* lens, int b, int N) { return t2_clamp_count(lens ? lens[b] : N, N); }

__global__ void __launch_bounds__(256) mel_l1_fwd_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                         const int* __restrict__ lens, int n_mel, int n, int N, long long RW,
                                                         int rpb, double count, float* __restrict__ partial) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * rpb;
    double acc = 0.0;
    for (int rr = 0; rr < rpb; ++rr) {
        const long long row = row0 + rr;
        if (row >= RW) break;
        const int len = ab_len(lens, (int)(row / n_mel), N);
        for (int i = tid; i < len; i += 256) acc += (double)fabsf(out[row * n + i] - target[row * N + i]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (float)(t2_block_total_f64(wsum) / count);
}

extern "C" int t2amd_mel_l1_rows_per_slot(int n) {
    if (n < 1) n = 1;
    return n >= 16384 ? 1 : (16384 + n - 1) / n;       // about 16k elements per workgroup
}

extern "C" int t2amd_mel_l1_fwd_f32(const float* out, const float* target, const int* lens, int B, int n_mel, int n, int N,
                                    long long count, float* partial, long long partial_floats, void* stream) {
    T2_REQUIRE(out && target && partial, "mel_l1_fwd: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && n_mel > 0 && n_mel <= 65535 && n > 0 && N > 0, "mel_l1_fwd: bad dims");
    T2_REQUIRE(N <= n, "mel_l1_fwd: the target has more frames than the prediction");
    T2_REQUIRE(count > 0 && count <= (long long)B * n_mel * N, "mel_l1_fwd: count must be n_mel times the frames inside the mask");
    const long long RW = (long long)B * n_mel;
    const int rpb = t2amd_mel_l1_rows_per_slot(n);
    const long long slots = (RW + rpb - 1) / rpb;
    T2_REQUIRE(partial_floats >= slots, "mel_l1_fwd: partial is shorter than its slots");
    T2_LAUNCH(mel_l1_fwd_kernel, dim3((unsigned)slots), dim3(256), 0, (hipStream_t)stream, out, target, lens, n_mel, n, N, RW, rpb,
              (double)count, partial);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// d_out[b][m][j] = sign(out - target) g[0] / count for j < lens[b], exactly 0 for every other j < n (g: the upstream scalar,
// read on the device so that no host synchronisation stands between the loss and its backward)
__global__ void __launch_bounds__(256) mel_l1_bwd_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                         const int* __restrict__ lens, const float* __restrict__ g, int n_mel,
                                                         int n, int N, long long total, float count,
                                                         float* __restrict__ d_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / n;
    const int j = (int)(i - row * n);
    float v = 0.0f;
    if (j < ab_len(lens, (int)(row / n_mel), N)) {
        const float d = out[i] - target[row * N + j], s = g[0] / count;
        v = d > 0.0f ? s : (d < 0.0f ? -s : 0.0f);
    }
    d_out[i] = v;
}

extern "C" int t2amd_mel_l1_bwd_f32(const float* out, const float* target, const int* lens, const float* g, int B, int n_mel,
                                    int n, int N, long long count, float* d_out, void* stream) {
    T2_REQUIRE(out && target && g && d_out, "mel_l1_bwd: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && n_mel > 0 && n_mel <= 65535 && n > 0 && N > 0, "mel_l1_bwd: bad dims");
    T2_REQUIRE(N <= n, "mel_l1_bwd: the target has more frames than the prediction");
    T2_REQUIRE(count > 0 && count <= (long long)B * n_mel * N, "mel_l1_bwd: count must be n_mel times the frames inside the mask");
    const long long total = (long long)B * n_mel * n, blocks = (total + 255) / 256;
    T2_REQUIRE(!t2_overlap(d_out, total * 4, out, total * 4) && !t2_overlap(d_out, total * 4, target, (long long)B * n_mel * N * 4),
               "mel_l1_bwd: d_out must not be one of the inputs");
    T2_REQUIRE(blocks <= 0x7fffffffLL, "mel_l1_bwd: too many elements for one launch");
    T2_LAUNCH(mel_l1_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, target, lens, g, n_mel, n, N, total,
              (float)count, d_out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
