// HiFi-GAN generator, the two element-wise ends of the path (the products are in hifigan.hip, which has the layout):
// hg_pack_mel: (B, n_mel, N) mels -> the stage-0 row image [P0][ldo] with zero halo rows and zero padding columns.
// hg_post: conv_post (C -> 1 channel, 7 taps, leaky-ReLU on the operand, tanh): one thread per row over an LDS window of
// 128 + 6 rows, written straight into the (B, 1, T) output through rowb0 / rowr0; halo rows are not written.
// No MFMA here, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define HG_POST_ROWS 128
#define HG_POST_TAPS 7
#define HG_POST_MAXC 64

__device__ __forceinline__ float hg_post_lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }

__global__ __launch_bounds__(HG_POST_ROWS) void hg_post_kernel(const float* X, long long ldx, long long P, int C, const float* w,
                                                               const float* bias, float slope, const int* rowb0,
                                                               const int* rowr0, int rdiv, float* out, long long T) {
    __shared__ float sx[(HG_POST_ROWS + HG_POST_TAPS - 1) * (HG_POST_MAXC + 1)];
    __shared__ float sw[HG_POST_TAPS * HG_POST_MAXC];
    const int ld = C + 1, win = HG_POST_ROWS + HG_POST_TAPS - 1;
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * HG_POST_ROWS;
    for (int i = tid; i < win * C; i += HG_POST_ROWS) {
        const int r = i / C, c = i - r * C;
        const long long src = row0 + r - (HG_POST_TAPS - 1) / 2;
        sx[r * ld + c] = (src >= 0 && src < P) ? hg_post_lrelu(X[src * ldx + c], slope) : 0.f;
    }
    for (int i = tid; i < HG_POST_TAPS * C; i += HG_POST_ROWS) sw[i] = w[i];
    __syncthreads();
    const long long gm = row0 + tid;
    if (gm >= P) return;
    const long long f = gm / rdiv;
    const int b = rowb0[f];
    if (b < 0) return;
    float acc = 0.f;
    for (int tap = 0; tap < HG_POST_TAPS; ++tap)
        for (int c = 0; c < C; ++c) acc = fmaf(sx[(tid + tap) * ld + c], sw[tap * C + c], acc);
    out[(long long)b * T + (long long)rowr0[f] * rdiv + (gm - f * rdiv)] = tanhf(acc + bias[0]);
}

extern "C" int t2amd_hg_post_f32(const float* X, long long x_floats, long long ldx, long long P, int C, const float* w,
                                 long long w_floats, const float* bias, float slope, const int* rowb0, const int* rowr0,
                                 long long n_rowb, int rdiv, float* out, long long T, long long out_floats, void* stream) {
    T2_REQUIRE(X && w && bias && rowb0 && rowr0 && out, "hg_post: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && C >= 1 && C <= HG_POST_MAXC, "hg_post: 1 to 64 input channels, at most 2^31 - 256 rows");
    T2_REQUIRE(ldx >= C && x_floats >= (P - 1) * ldx + C, "hg_post: X is shorter than its rows");
    T2_REQUIRE(w_floats >= HG_POST_TAPS * C, "hg_post: w is shorter than [7][C]");
    T2_REQUIRE(rdiv >= 1 && P % rdiv == 0 && n_rowb >= P / rdiv, "hg_post: the row map does not cover the rows");
    T2_REQUIRE(T >= 1 && out_floats >= T, "hg_post: out is shorter than one utterance");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(X) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
               "hg_post: X / out misaligned");
    T2_LAUNCH(hg_post_kernel, dim3(t2_cdiv(P, HG_POST_ROWS)), dim3(HG_POST_ROWS), 0, (hipStream_t)stream, X, ldx, P, C, w, bias,
              slope, rowb0, rowr0, rdiv, out, T);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

__global__ __launch_bounds__(256) void hg_pack_mel_kernel(const float* mel, int n_mel, long long N, const int* rowb0,
                                                          const int* rowr0, long long P0, float* out, int ldo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P0 * ldo) return;
    const long long p = i / ldo;
    const int c = (int)(i - p * ldo);
    const int b = rowb0[p];
    out[i] = (b >= 0 && c < n_mel) ? mel[((long long)b * n_mel + c) * N + rowr0[p]] : 0.f;
}

extern "C" int t2amd_hg_pack_mel_f32(const float* mel, long long mel_floats, int B, int n_mel, long long N, const int* rowb0,
                                     const int* rowr0, long long P0, float* out, int ldo, long long out_floats, void* stream) {
    T2_REQUIRE(mel && rowb0 && rowr0 && out, "hg_pack_mel: null operand");
    T2_REQUIRE(B >= 1 && n_mel >= 1 && N >= 1 && P0 >= 1, "hg_pack_mel: bad dims");
    T2_REQUIRE(mel_floats >= (long long)B * n_mel * N, "hg_pack_mel: mel is shorter than (B, n_mel, N)");
    T2_REQUIRE(ldo >= n_mel && ldo % 4 == 0 && t2_aligned16(out), "hg_pack_mel: out rows must be 16-byte aligned and hold n_mel");
    T2_REQUIRE(out_floats >= P0 * ldo && P0 * ldo <= T2_MAX_ROWS * 64, "hg_pack_mel: out is shorter than its rows");
    T2_LAUNCH(hg_pack_mel_kernel, dim3(t2_cdiv(P0 * ldo, 256)), dim3(256), 0, (hipStream_t)stream, mel, n_mel, N, rowb0, rowr0, P0,
              out, ldo);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
