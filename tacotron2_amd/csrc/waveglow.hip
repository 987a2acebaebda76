// WaveGlow inference on the GPU (tacotron2_amd/waveglow.py): the element passes of the flow loop.  The products run
// elsewhere: the upsample and the per-flow cond product on gemm.hip's t2amd_gemm_f32, the two WN layer products on
// waveglow_layer.hip's t2amd_wg_layer_f32.  What is here is plain C++ (expf, no builtins) so that the CPU test-suite can
// run these very kernels through tests/hip_emu.
//
// Packed row space.  Row r of utterance b holds samples n_group * r .. n_group * r + n_group - 1 (R_b = n_b * hop / n_group
// rows).  Every utterance's rows sit in one packed row space between zero halos of `halo` rows
// ((kernel_size - 1) / 2 * 2^(L-1): the deepest dilated tap), [halo | R_0 | halo | R_1 | ... | R_{B-1} | halo], so dilated
// taps never cross utterances and need no bounds test.  `rowb[p]` is the utterance of packed row p (-1 for a halo row),
// `rowr[p]` its row within that utterance.  Halo rows of the image h are zero and are never written.
//
// State between launches, all channel-last f32 rows: h [P][C] (the WN input image), acts [P][C], skip [P][C], audio
// [P][ldaudio] (the channels of the flow currently being inverted).
#include "common.h"

#define WG_ROWS 32           // rows per workgroup of the flow tail
#define WG_MAXC 512          // WN channels
#define WG_MAXG 16           // n_group

// Flow tail for the packed rows [p0, p0 + 32) of one workgroup (256 threads), for every row p with rowb[p] >= 0:
//   e = end_b + end_w . skip[p]                            (end_w [n_in][C]; skipped when end_w == NULL: the first call)
//   x1 = (x1 - e[:n_in/2]) / exp(e[n_in/2:]),  y = winv . [x0; x1]      (x = audio[p][0:n_in])
//   a = [sigma * z[b][0:n_new][r] ; y]                     (z == NULL: a = y)
//   out[b][n_group r + g] = a[g]   when `out` is set, else audio[p][0:n_out] = a
//   h[p][c] = start_b[c] + start_w[c] . a[0:n_out/2]       when start_w is set (the next flow's start)
__global__ void __launch_bounds__(256) wg_tail_kernel(
    const float* __restrict__ skip, long long ldskip, int C, const float* __restrict__ end_w, const float* __restrict__ end_b,
    int n_in, const float* __restrict__ winv, float* __restrict__ audio, long long ldaudio, const float* __restrict__ z,
    long long zb, long long zc, int n_new, float sigma, const float* __restrict__ start_w, const float* __restrict__ start_b,
    float* __restrict__ h, long long ldh, float* __restrict__ out, long long ldout, const int* __restrict__ rowb,
    const int* __restrict__ rowr, long long P, int n_group) {
    __shared__ float s_end[WG_MAXG * WG_MAXC];
    __shared__ float s_start[WG_MAXC * (WG_MAXG / 2)];
    __shared__ float s_winv[WG_MAXG * WG_MAXG];
    __shared__ float s_e[WG_ROWS][WG_MAXG];
    __shared__ float s_a[WG_ROWS][WG_MAXG];
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * WG_ROWS;
    const int n_cur = end_w ? n_in : 0;
    const int n_out = n_cur + (z ? n_new : 0);
    const int nh_next = n_out / 2;
    if (end_w) {
        for (int i = tid; i < n_in * C; i += 256) s_end[i] = end_w[i];
        for (int i = tid; i < n_in * n_in; i += 256) s_winv[i] = winv[i];
    }
    if (start_w)
        for (int i = tid; i < C * nh_next; i += 256) s_start[i] = start_w[i];
    __syncthreads();

    // end product: thread -> (row, output), 8 outputs per row in flight
    if (end_w) {
        const int row = tid >> 3;
        const long long p = p0 + row;
        if (p < P && rowb[p] >= 0) {
            const float* sr = skip + p * ldskip;
            for (int o = tid & 7; o < n_in; o += 8) {
                const float* w = s_end + o * C;
                float acc = 0.0f;
                for (int c = 0; c < C; ++c) acc += sr[c] * w[c];
                s_e[row][o] = acc + end_b[o];
            }
        }
    }
    __syncthreads();

    // affine inverse, 1x1 mix, noise insertion: one thread per row
    if (tid < WG_ROWS) {
        const int row = tid;
        const long long p = p0 + row;
        if (p < P && rowb[p] >= 0) {
            const int b = rowb[p];
            const long long r = rowr[p];
            float x[WG_MAXG], y[WG_MAXG];
            const int nh = n_cur / 2;
            for (int j = 0; j < n_cur; ++j) x[j] = audio[p * ldaudio + j];
            for (int j = 0; j < nh; ++j) x[nh + j] = (x[nh + j] - s_e[row][j]) / expf(s_e[row][nh + j]);
            for (int i = 0; i < n_cur; ++i) {
                float acc = 0.0f;
                for (int j = 0; j < n_cur; ++j) acc += s_winv[i * n_cur + j] * x[j];
                y[i] = acc;
            }
            float* a = s_a[row];
            int k = 0;
            if (z)
                for (; k < n_new; ++k) a[k] = sigma * z[b * zb + k * zc + r];
            for (int i = 0; i < n_cur; ++i) a[k + i] = y[i];
            if (out) {
                for (int g = 0; g < n_out; ++g) out[b * ldout + r * n_group + g] = a[g];
            } else {
                for (int g = 0; g < n_out; ++g) audio[p * ldaudio + g] = a[g];
            }
        }
    }
    __syncthreads();

    // the next flow's start: thread -> channel, coalesced rows
    if (start_w) {
        for (int c = tid; c < C; c += 256) {
            float w[WG_MAXG / 2];
            for (int j = 0; j < nh_next; ++j) w[j] = s_start[c * nh_next + j];
            const float bc = start_b[c];
            for (int row = 0; row < WG_ROWS; ++row) {
                const long long p = p0 + row;
                if (p >= P || rowb[p] < 0) continue;
                float acc = 0.0f;
                for (int j = 0; j < nh_next; ++j) acc += w[j] * s_a[row][j];
                h[p * ldh + c] = acc + bc;
            }
        }
    }
}

extern "C" int t2amd_wg_tail_f32(const float* skip, long long ldskip, int C, const float* end_w, const float* end_b, int n_in,
                                 const float* winv, float* audio, long long ldaudio, const float* z, long long zb,
                                 long long zc, int n_new, float sigma, const float* start_w, const float* start_b, float* h,
                                 long long ldh, float* out, long long ldout, const int* rowb, const int* rowr, long long P,
                                 int n_group, void* stream) {
    T2_REQUIRE(rowb && rowr && audio, "wg_tail: null operand");
    T2_REQUIRE(P > 0, "wg_tail: no rows");
    T2_REQUIRE(C <= WG_MAXC && (C > 0 || (!end_w && !start_w)), "wg_tail: C must be in 1..512");
    T2_REQUIRE(n_group >= 2 && n_group <= WG_MAXG && n_group % 2 == 0, "wg_tail: n_group must be even and at most 16");
    T2_REQUIRE(ldaudio >= n_group, "wg_tail: audio rows too short");
    if (end_w) {
        T2_REQUIRE(skip && end_b && winv, "wg_tail: null operand");
        T2_REQUIRE(n_in >= 2 && n_in % 2 == 0 && n_in <= n_group, "wg_tail: n_in must be even and at most n_group");
        T2_REQUIRE(ldskip >= C, "wg_tail: skip rows too short");
    } else {
        T2_REQUIRE(z != nullptr, "wg_tail: the first call needs the noise");
    }
    const int n_cur = end_w ? n_in : 0;
    if (z) T2_REQUIRE(n_new >= 1 && zc >= 1 && zb >= (long long)n_new * zc, "wg_tail: bad noise strides");
    const int n_out = n_cur + (z ? n_new : 0);
    T2_REQUIRE(n_out >= 2 && n_out % 2 == 0 && n_out <= n_group, "wg_tail: channel count out of range");
    if (start_w) T2_REQUIRE(start_b && h && ldh >= C, "wg_tail: start needs start_b and h");
    if (out) {
        T2_REQUIRE(n_out == n_group, "wg_tail: the waveform needs all n_group channels");
        T2_REQUIRE(!start_w, "wg_tail: the last flow has no next start");
        T2_REQUIRE(ldout >= n_group, "wg_tail: waveform rows too short");
    }
    const long long nblk = (P + WG_ROWS - 1) / WG_ROWS;
    T2_REQUIRE(nblk <= 0x7fffffffLL, "wg_tail: too many rows");
    T2_LAUNCH(wg_tail_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, skip, ldskip, C, end_w, end_b, n_in,
              winv, audio, ldaudio, z, zb, zc, n_new, sigma, start_w, start_b, h, ldh, out, ldout, rowb, rowr, P, n_group);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// Denoiser: mag[b][f][t] = max(mag - bias[f] * strength, 0) in place (reference denoiser.py forward, the clamp keeps NaN).
__global__ void __launch_bounds__(256) wg_denoise_kernel(float* __restrict__ mag, const float* __restrict__ bias, int F,
                                                         long long n, float strength, long long total) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int f = (int)((i / n) % F);
        const float v = mag[i] - __fmul_rn(bias[f], strength);       // two roundings, like torch
        mag[i] = v < 0.0f ? 0.0f : v;
    }
}

extern "C" int t2amd_wg_denoise_f32(float* mag, const float* bias, int B, int F, long long n, float strength, void* stream) {
    T2_REQUIRE(mag && bias, "wg_denoise: null operand");
    T2_REQUIRE(B > 0 && F > 0 && n > 0, "wg_denoise: bad dims");
    const long long total = (long long)B * F * n;
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    T2_LAUNCH(wg_denoise_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mag, bias, F, n, strength, total);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
