// WaveGlow's forward direction on the GPU (tacotron2_amd/waveglow.py: WaveGlow.forward, WaveGlow.nll, WaveGlowLoss): audio
// to latents and the terms of the negative log-likelihood.  The products are the ones inference runs (t2amd_gemm_f32,
// t2amd_wg_layer_f32: WN is the same function of (audio_0, cond) in both directions); what is here is the element work
// between them, the mirror image of waveglow.hip's flow tail, and the loss reduction.  Plain C++ (expf, no builtins, no
// atomics) so that the CPU test-suite can run these very kernels through tests/hip_emu.
//
// The packed row space, rowb / rowr and the state between launches (h, skip, audio rows) are waveglow.hip's.
#include "common.h"

#define WG_ROWS 32           // rows per workgroup of the flow head
#define WG_MAXC 512          // WN channels
#define WG_MAXG 16           // n_group
#define WG_NLL_CHUNK 2048    // rows of one utterance per workgroup of the reduction's first stage

// Flow head for the packed rows [p0, p0 + 32) of one workgroup (256 threads), for every row p with rowb[p] >= 0
// (b = rowb[p], r = rowr[p]); it closes flow k and opens flow k + 1:
//   x = audio[p][0:n_in],  e = end_b + end_w . skip[p]       (end_w [n_in][C])
//   x1 = exp(e[n_in/2:]) * x1 + e[:n_in/2],  log_s[b][j][r] = e[n_in/2 + j]
//     (end_w == NULL, the first call: x[g] = wave[b][n_group r + g], n_in = n_group channels, no flow to close)
//   z[b][z_off + k][r] = x[k] for k < n_emit                 (an early output; everything that is left on the last call)
//   a = mix_w . x[n_emit:],  audio[p][0:n_out] = a           (mix_w [n_out][n_out], n_out = n_in - n_emit; NULL: the last call)
//   h[p][c] = start_b[c] + start_w[c] . a[0:n_out/2]         (the next flow's start)
// sv != NULL (the training forward): sv[p][0:n_cur] = x and sv[p][n_group:n_group + n_out] = a are kept for the backward pass.
__global__ void __launch_bounds__(256) wg_head_kernel(
    const float* __restrict__ skip, long long ldskip, int C, const float* __restrict__ end_w, const float* __restrict__ end_b,
    int n_in, float* __restrict__ log_s, long long lsb, long long lsc, const float* __restrict__ wave, long long ldwave,
    float* __restrict__ audio, long long ldaudio, float* __restrict__ z, long long zb, long long zc, int z_off, int n_emit,
    const float* __restrict__ mix_w, const float* __restrict__ start_w, const float* __restrict__ start_b,
    float* __restrict__ h, long long ldh, const int* __restrict__ rowb, const int* __restrict__ rowr, long long P, int n_group,
    int B, long long R, float* __restrict__ sv, long long ldsv) {
    __shared__ float s_end[WG_MAXG * WG_MAXC];
    __shared__ float s_start[WG_MAXC * (WG_MAXG / 2)];
    __shared__ float s_mix[WG_MAXG * WG_MAXG];
    __shared__ float s_e[WG_ROWS][WG_MAXG];
    __shared__ float s_a[WG_ROWS][WG_MAXG];
    __shared__ int s_ok[WG_ROWS];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * WG_ROWS;
    const int n_cur = end_w ? n_in : n_group;
    const int n_out = n_cur - n_emit;
    const int nh_next = n_out / 2;
    if (end_w)
        for (int i = tid; i < n_in * C; i += 256) s_end[i] = end_w[i];
    if (mix_w) {
        for (int i = tid; i < n_out * n_out; i += 256) s_mix[i] = mix_w[i];
        for (int i = tid; i < C * nh_next; i += 256) s_start[i] = start_w[i];
    }
    if (tid < WG_ROWS) {
        const long long p = p0 + tid;
        s_ok[tid] = p < P && rowb[p] >= 0 && rowb[p] < B && rowr[p] >= 0 && rowr[p] < R;
    }
    __syncthreads();

    // end product: thread -> (row, output), 8 outputs per row in flight
    if (end_w) {
        const int row = tid >> 3;
        if (s_ok[row]) {
            const float* sr = skip + (p0 + row) * ldskip;
            for (int o = tid & 7; o < n_in; o += 8) {
                const float* w = s_end + o * C;
                float acc = 0.0f;
                for (int c = 0; c < C; ++c) acc += sr[c] * w[c];
                s_e[row][o] = acc + end_b[o];
            }
        }
    }
    __syncthreads();

    // affine coupling, log_s, early output, the next flow's 1x1 mix: one thread per row
    if (tid < WG_ROWS && s_ok[tid]) {
        const int row = tid;
        const long long p = p0 + row;
        const long long b = rowb[p];
        const long long r = rowr[p];
        float x[WG_MAXG];
        if (end_w) {
            const int nh = n_in / 2;
            for (int j = 0; j < n_in; ++j) x[j] = audio[p * ldaudio + j];
            for (int j = 0; j < nh; ++j) {
                const float ls = s_e[row][nh + j];
                x[nh + j] = expf(ls) * x[nh + j] + s_e[row][j];
                log_s[b * lsb + j * lsc + r] = ls;
            }
        } else {
            for (int g = 0; g < n_group; ++g) x[g] = wave[b * ldwave + r * n_group + g];
        }
        for (int k = 0; k < n_emit; ++k) z[b * zb + (z_off + k) * zc + r] = x[k];
        if (sv)
            for (int k = 0; k < n_cur; ++k) sv[p * ldsv + k] = x[k];
        if (mix_w) {
            for (int i = 0; i < n_out; ++i) {
                float acc = 0.0f;
                for (int j = 0; j < n_out; ++j) acc += s_mix[i * n_out + j] * x[n_emit + j];
                s_a[row][i] = acc;
                audio[p * ldaudio + i] = acc;
                if (sv) sv[p * ldsv + n_group + i] = acc;
            }
        }
    }
    __syncthreads();

    // the next flow's start: thread -> channel, coalesced rows
    if (mix_w) {
        for (int c = tid; c < C; c += 256) {
            float w[WG_MAXG / 2];
            for (int j = 0; j < nh_next; ++j) w[j] = s_start[c * nh_next + j];
            const float bc = start_b[c];
            for (int row = 0; row < WG_ROWS; ++row) {
                if (!s_ok[row]) continue;
                float acc = 0.0f;
                for (int j = 0; j < nh_next; ++j) acc += w[j] * s_a[row][j];
                h[(p0 + row) * ldh + c] = acc + bc;
            }
        }
    }
}

extern "C" int t2amd_wg_head_save_f32(const float* skip, long long ldskip, int C, const float* end_w, const float* end_b,
                                      int n_in, float* log_s, long long lsb, long long lsc, const float* wave, long long ldwave,
                                      float* audio, long long ldaudio, float* z, long long zb, long long zc, int z_off,
                                      int n_emit, const float* mix_w, const float* start_w, const float* start_b, float* h,
                                      long long ldh, const int* rowb, const int* rowr, long long P, int n_group, int B,
                                      long long R, float* sv, long long ldsv, void* stream) {
    T2_REQUIRE(!sv || ldsv >= 2 * n_group, "wg_head: saved rows hold 2 n_group values");
    T2_REQUIRE(rowb && rowr && audio, "wg_head: null operand");
    T2_REQUIRE(P > 0 && B > 0 && R > 0, "wg_head: no rows");
    T2_REQUIRE(C > 0 && C <= WG_MAXC, "wg_head: C must be in 1..512");
    T2_REQUIRE(n_group >= 2 && n_group <= WG_MAXG && n_group % 2 == 0, "wg_head: n_group must be even and at most 16");
    T2_REQUIRE(ldaudio >= n_group, "wg_head: audio rows too short");
    T2_REQUIRE((end_w != nullptr) != (wave != nullptr), "wg_head: either a flow to close (end_w) or the waveform");
    if (end_w) {
        T2_REQUIRE(skip && end_b && log_s, "wg_head: null operand");
        T2_REQUIRE(n_in >= 2 && n_in % 2 == 0 && n_in <= n_group, "wg_head: n_in must be even and at most n_group");
        T2_REQUIRE(ldskip >= C, "wg_head: skip rows too short");
        T2_REQUIRE(lsc >= R && lsb >= (long long)(n_in / 2) * lsc, "wg_head: bad log_s strides");
    } else {
        T2_REQUIRE(ldwave >= R * n_group, "wg_head: waveform rows too short");
    }
    const int n_cur = end_w ? n_in : n_group;
    T2_REQUIRE(n_emit >= 0 && n_emit % 2 == 0 && n_emit <= n_cur, "wg_head: n_emit must be even and at most the channels held");
    if (n_emit > 0) {
        T2_REQUIRE(z != nullptr, "wg_head: an early output needs z");
        T2_REQUIRE(z_off >= 0 && z_off + n_emit <= n_group, "wg_head: the early output leaves z's channels");
        T2_REQUIRE(zc >= R && zb >= (long long)n_group * zc, "wg_head: bad z strides");
    }
    const int n_out = n_cur - n_emit;
    if (mix_w) {
        T2_REQUIRE(n_out >= 2, "wg_head: the next flow needs at least 2 channels");
        T2_REQUIRE(start_w && start_b && h && ldh >= C, "wg_head: the next flow needs start_w, start_b and h");
    } else {
        T2_REQUIRE(n_out == 0, "wg_head: the last call writes every remaining channel to z");
        T2_REQUIRE(!start_w, "wg_head: the last flow has no next start");
    }
    const long long nblk = (P + WG_ROWS - 1) / WG_ROWS;
    T2_REQUIRE(nblk <= 0x7fffffffLL, "wg_head: too many rows");
    T2_LAUNCH(wg_head_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, skip, ldskip, C, end_w, end_b, n_in,
              log_s, lsb, lsc, wave, ldwave, audio, ldaudio, z, zb, zc, z_off, n_emit, mix_w, start_w, start_b, h, ldh, rowb,
              rowr, P, n_group, B, R, sv, ldsv);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_wg_head_f32(const float* skip, long long ldskip, int C, const float* end_w, const float* end_b, int n_in,
                                 float* log_s, long long lsb, long long lsc, const float* wave, long long ldwave,
                                 float* audio, long long ldaudio, float* z, long long zb, long long zc, int z_off, int n_emit,
                                 const float* mix_w, const float* start_w, const float* start_b, float* h, long long ldh,
                                 const int* rowb, const int* rowr, long long P, int n_group, int B, long long R,
                                 void* stream) {
    return t2amd_wg_head_save_f32(skip, ldskip, C, end_w, end_b, n_in, log_s, lsb, lsc, wave, ldwave, audio, ldaudio, z, zb, zc,
                                  z_off, n_emit, mix_w, start_w, start_b, h, ldh, rowb, rowr, P, n_group, B, R, nullptr, 0, stream);
}

// The two sums of the negative log-likelihood per utterance, in a fixed order (two stages, no atomics): the numbers of an
// utterance depend on its own rows alone, not on the batch around it.
// Stage 1, workgroup (chunk, b): rows [2048 chunk, 2048 (chunk + 1)) below len[b]; thread t takes rows t, t + 256, ... of the
// chunk, channel after channel, in double; a tree over the 256 threads -> partial[b][chunk][0:2] = {sum z^2, sum log_s}.
__device__ __forceinline__ void wg_nll_tree(double (*s)[2], int tid) {
    for (int step = 128; step > 0; step >>= 1) {
        __syncthreads();
        if (tid < step) {
            s[tid][0] += s[tid + step][0];
            s[tid][1] += s[tid + step][1];
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) wg_nll_partial_kernel(const float* __restrict__ z, long long zb, long long zc, int nz,
                                                             const float* __restrict__ ls, long long lb, long long lc, int nls,
                                                             const int* __restrict__ len, long long R,
                                                             double* __restrict__ partial, long long nchunk) {
    __shared__ double s[256][2];
    const int tid = threadIdx.x;
    const long long b = blockIdx.y;
    const long long chunk = blockIdx.x;
    long long n = len[b];
    n = n < 0 ? 0 : (n > R ? R : n);
    const long long r0 = chunk * WG_NLL_CHUNK;
    const long long r1 = r0 + WG_NLL_CHUNK < n ? r0 + WG_NLL_CHUNK : n;
    double zz = 0.0, sl = 0.0;
    for (int c = 0; c < nz; ++c) {
        const float* src = z + b * zb + c * zc;
        for (long long r = r0 + tid; r < r1; r += 256) {
            const double v = (double)src[r];
            zz += v * v;
        }
    }
    for (int c = 0; c < nls; ++c) {
        const float* src = ls + b * lb + c * lc;
        for (long long r = r0 + tid; r < r1; r += 256) sl += (double)src[r];
    }
    s[tid][0] = zz;
    s[tid][1] = sl;
    wg_nll_tree(s, tid);
    if (tid == 0) {
        partial[(b * nchunk + chunk) * 2] = s[0][0];
        partial[(b * nchunk + chunk) * 2 + 1] = s[0][1];
    }
}

// Stage 2, workgroup b: the chunks below len[b] in a fixed order -> out[b][0:2].
__global__ void __launch_bounds__(256) wg_nll_final_kernel(const double* __restrict__ partial, long long nchunk,
                                                           const int* __restrict__ len, long long R, double* __restrict__ out) {
    __shared__ double s[256][2];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    long long n = len[b];
    n = n < 0 ? 0 : (n > R ? R : n);
    const long long nc = (n + WG_NLL_CHUNK - 1) / WG_NLL_CHUNK;
    double zz = 0.0, sl = 0.0;
    for (long long c = tid; c < nc; c += 256) {
        zz += partial[(b * nchunk + c) * 2];
        sl += partial[(b * nchunk + c) * 2 + 1];
    }
    s[tid][0] = zz;
    s[tid][1] = sl;
    wg_nll_tree(s, tid);
    if (tid == 0) {
        out[b * 2] = s[0][0];
        out[b * 2 + 1] = s[0][1];
    }
}

extern "C" int t2amd_wg_nll_chunk(void) { return WG_NLL_CHUNK; }

extern "C" int t2amd_wg_nll_f32(const float* z, long long zb, long long zc, int nz, const float* ls, long long lb, long long lc,
                                int nls, const int* len, int B, long long R, double* partial, long long nchunk, double* out,
                                void* stream) {
    T2_REQUIRE(z && len && partial && out, "wg_nll: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && R > 0, "wg_nll: bad dims");
    T2_REQUIRE(nz >= 1 && zc >= R && zb >= (long long)nz * zc, "wg_nll: bad z strides");
    T2_REQUIRE(nls >= 0 && (nls == 0 || ls != nullptr), "wg_nll: null operand");
    if (nls > 0) T2_REQUIRE(lc >= R && lb >= (long long)nls * lc, "wg_nll: bad log_s strides");
    T2_REQUIRE(nchunk == (R + WG_NLL_CHUNK - 1) / WG_NLL_CHUNK, "wg_nll: partial needs ceil(R / chunk) entries per utterance");
    T2_REQUIRE(nchunk <= 0x7fffffffLL, "wg_nll: too many rows");
    T2_LAUNCH(wg_nll_partial_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, z, zb, zc, nz, ls,
              lb, lc, nls, len, R, partial, nchunk);
    T2_LAUNCH_CHECK();
    T2_LAUNCH(wg_nll_final_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, partial, nchunk, len, R, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
