// WaveGlow's backward pass on the GPU (tacotron2_amd/waveglow.py: WaveGlow.training_loss): the element work between the
// gradient products.  The products themselves run on t2amd_gemm_f32 (weight gradients, split-K) and on mode 2 of
// t2amd_wg_layer_train_f32 (the dilated data gradient); what is here is the mirror image of waveglow_fwd.hip's flow head,
// the gate's backward and the fixed-order reduction of the head's small parameter gradients.  Plain C++ (expf, no
// builtins, no atomics) so that the CPU test-suite can run these very kernels through tests/hip_emu; two runs give
// identical bits.
//
// The packed row space, rowb / rowr and the per-call saved state (x | a rows, skip, log_s) are waveglow_fwd.hip's.
#include "common.h"

#define WGB_ROWS 32          // rows per pass of a workgroup of the head backward
#define WGB_SUB 2            // passes per workgroup: 64 rows share one set of partial sums
#define WG_MAXC 512          // WN channels
#define WG_MAXG 16           // n_group

// Backward of the flow head call that closed flow k (end_w, n_in channels) and opened flow k + 1 (mix_w, n_out = n_cur -
// n_emit channels), for every real row p (b = rowb[p], r = rowr[p]); loss = (sum z^2 / (2 sigma^2) - sum log_s - ...) / numel,
// c1 = 1 / (sigma^2 numel), c2 = -1 / numel:
//   da = dA[p][0:n_out];  da[0:n_out/2] += start_w^T . dh0[p]            (dh0: gradient of the next flow's layer-0 input)
//   partial d_start_w[c][j] += dh0[p][c] a[p][j],  d_start_b[c] += dh0[p][c]      (a = a_sv: the mixed rows the head wrote)
//   dx[n_emit:] = mix_w^T . da,  partial d_mix[o][i] += da[o] x[p][n_emit + i]    (x = x_sv: the rows before the mix)
//   dx[k] = c1 x[p][k] for k < n_emit                                    (the early output is z itself)
//   coupling x1' = exp(s) x1 + b:  de = [dx1', dx1' x1 exp(s) + c2],  dA[p] = [dx0, dx1' exp(s)]   (x1 = a_in[p][n_in/2:])
//   d_skip[p] = end_w^T . de,  partial d_end_w[o][c] += de[o] skip[p][c],  d_end_b[o] += de[o]
// end_w == NULL is the first call (the waveform: nothing to close, dx is dropped), mix_w == NULL the last one (n_out = 0).
// Each workgroup stores its partial sums [end_w | end_b | start_w | start_b | mix] at partial + blockIdx.x * npart;
// t2amd_wg_partial_sum_f32 adds them in block order.
__global__ void __launch_bounds__(256) wg_head_bwd_kernel(
    const float* __restrict__ skip, long long ldskip, int C, const float* __restrict__ end_w, int n_in,
    const float* __restrict__ log_s, long long lsb, long long lsc, const float* __restrict__ a_in, long long ldain,
    const float* __restrict__ x_sv, long long ldx, const float* __restrict__ a_sv, long long ldasv, float* __restrict__ dA,
    long long lddA, const float* __restrict__ dh0, long long lddh, const float* __restrict__ mix_w,
    const float* __restrict__ start_w, int n_emit, float* __restrict__ d_skip, long long ldds, float* __restrict__ partial,
    long long npart, const int* __restrict__ rowb, const int* __restrict__ rowr, long long P, int n_group, int B, long long R,
    float c1, float c2) {
    __shared__ float s_start[WG_MAXC * (WG_MAXG / 2)];
    __shared__ float s_mix[WG_MAXG * WG_MAXG];
    __shared__ float s_g[WGB_ROWS][WG_MAXG / 2];
    __shared__ float s_de[WGB_ROWS][WG_MAXG];
    __shared__ float s_da[WGB_ROWS][WG_MAXG];
    __shared__ float s_x[WGB_ROWS][WG_MAXG];
    __shared__ float s_a[WGB_ROWS][WG_MAXG / 2];
    __shared__ int s_ok[WGB_ROWS];
    const int tid = threadIdx.x;
    const int n_cur = end_w ? n_in : n_group;
    const int n_out = n_cur - n_emit;
    const int nh_next = n_out / 2;
    const int nh = n_in / 2;
    if (mix_w) {
        for (int i = tid; i < n_out * n_out; i += 256) s_mix[i] = mix_w[i];
        for (int i = tid; i < C * nh_next; i += 256) s_start[i] = start_w[i];
    }
    float accE[2][WG_MAXG], accS[2][WG_MAXG / 2], accSb[2];
    for (int ci = 0; ci < 2; ++ci) {
        for (int o = 0; o < WG_MAXG; ++o) accE[ci][o] = 0.0f;
        for (int j = 0; j < WG_MAXG / 2; ++j) accS[ci][j] = 0.0f;
        accSb[ci] = 0.0f;
    }
    float accEb = 0.0f, accM = 0.0f;

    for (int sub = 0; sub < WGB_SUB; ++sub) {
        const long long p0 = ((long long)blockIdx.x * WGB_SUB + sub) * WGB_ROWS;
        __syncthreads();
        if (tid < WGB_ROWS) {
            const long long p = p0 + tid;
            s_ok[tid] = p < P && rowb[p] >= 0 && rowb[p] < B && rowr[p] >= 0 && rowr[p] < R;
        }
        __syncthreads();

        // through the next flow's start: thread -> (row, audio channel)
        if (mix_w) {
            const int row = tid >> 3, j = tid & 7;
            if (j < nh_next) {
                float acc = 0.0f;
                if (s_ok[row]) {
                    const float* g = dh0 + (p0 + row) * lddh;
                    for (int c = 0; c < C; ++c) acc += s_start[c * nh_next + j] * g[c];
                }
                s_g[row][j] = acc;
            }
        }
        __syncthreads();

        // the 1x1 mix, the early output and the affine coupling: one thread per row
        if (tid < WGB_ROWS) {
            const int row = tid;
            for (int o = 0; o < WG_MAXG; ++o) {
                s_de[row][o] = 0.0f;
                s_da[row][o] = 0.0f;
                s_x[row][o] = 0.0f;
            }
            for (int j = 0; j < WG_MAXG / 2; ++j) s_a[row][j] = 0.0f;
            if (s_ok[row]) {
                const long long p = p0 + row;
                const long long b = rowb[p];
                const long long r = rowr[p];
                float xv[WG_MAXG], dx[WG_MAXG];
                for (int k = 0; k < n_cur; ++k) xv[k] = x_sv[p * ldx + k];
                for (int k = 0; k < n_emit; ++k) dx[k] = xv[k] * c1;
                if (mix_w) {
                    float da[WG_MAXG];
                    for (int o = 0; o < n_out; ++o) {
                        da[o] = dA[p * lddA + o] + (o < nh_next ? s_g[row][o] : 0.0f);
                        s_da[row][o] = da[o];
                        s_x[row][o] = xv[n_emit + o];
                    }
                    for (int j = 0; j < nh_next; ++j) s_a[row][j] = a_sv[p * ldasv + j];
                    for (int i = 0; i < n_out; ++i) {
                        float acc = 0.0f;
                        for (int o = 0; o < n_out; ++o) acc += s_mix[o * n_out + i] * da[o];
                        dx[n_emit + i] = acc;
                    }
                }
                if (end_w) {
                    for (int j = 0; j < nh; ++j) {
                        const float es = expf(log_s[b * lsb + j * lsc + r]);
                        const float x1 = a_in[p * ldain + nh + j];
                        const float g1 = dx[nh + j];
                        s_de[row][j] = g1;
                        s_de[row][nh + j] = g1 * x1 * es + c2;
                        dA[p * lddA + j] = dx[j];
                        dA[p * lddA + nh + j] = g1 * es;
                    }
                }
            }
        }
        __syncthreads();

        // through end (d_skip, d_end_w) and the start's weight gradient: thread -> channel, coalesced rows
        for (int ci = 0; ci < 2; ++ci) {
            const int c = tid + 256 * ci;
            if (c >= C) break;
            if (end_w) {
                float w[WG_MAXG];
                for (int o = 0; o < n_in; ++o) w[o] = end_w[o * C + c];
                for (int row = 0; row < WGB_ROWS; ++row) {
                    if (!s_ok[row]) continue;
                    const float sk = skip[(p0 + row) * ldskip + c];
                    float acc = 0.0f;
                    for (int o = 0; o < n_in; ++o) {
                        acc += w[o] * s_de[row][o];
                        accE[ci][o] += s_de[row][o] * sk;
                    }
                    d_skip[(p0 + row) * ldds + c] = acc;
                }
            }
            if (mix_w) {
                for (int row = 0; row < WGB_ROWS; ++row) {
                    if (!s_ok[row]) continue;
                    const float g = dh0[(p0 + row) * lddh + c];
                    accSb[ci] += g;
                    for (int j = 0; j < nh_next; ++j) accS[ci][j] += g * s_a[row][j];
                }
            }
        }
        if (end_w && tid < n_in)
            for (int row = 0; row < WGB_ROWS; ++row) accEb += s_de[row][tid];
        if (mix_w && tid < n_out * n_out) {
            const int o = tid / n_out, i = tid - o * n_out;
            for (int row = 0; row < WGB_ROWS; ++row) accM += s_da[row][o] * s_x[row][i];
        }
    }

    float* out = partial + (long long)blockIdx.x * npart;
    long long off = 0;
    if (end_w) {
        for (int ci = 0; ci < 2; ++ci) {
            const int c = tid + 256 * ci;
            if (c < C)
                for (int o = 0; o < n_in; ++o) out[off + (long long)o * C + c] = accE[ci][o];
        }
        off += (long long)n_in * C;
        if (tid < n_in) out[off + tid] = accEb;
        off += n_in;
    }
    if (mix_w) {
        for (int ci = 0; ci < 2; ++ci) {
            const int c = tid + 256 * ci;
            if (c < C) {
                for (int j = 0; j < nh_next; ++j) out[off + (long long)c * nh_next + j] = accS[ci][j];
                out[off + (long long)C * nh_next + c] = accSb[ci];
            }
        }
        off += (long long)C * nh_next + C;
        if (tid < n_out * n_out) out[off + tid] = accM;
    }
}

extern "C" int t2amd_wg_head_bwd_rows(void) { return WGB_ROWS * WGB_SUB; }

extern "C" int t2amd_wg_head_bwd_f32(const float* skip, long long ldskip, int C, const float* end_w, int n_in, const float* log_s,
                                     long long lsb, long long lsc, const float* a_in, long long ldain, const float* x_sv,
                                     long long ldx, const float* a_sv, long long ldasv, float* dA, long long lddA,
                                     const float* dh0, long long lddh, const float* mix_w, const float* start_w, int n_emit,
                                     float* d_skip, long long ldds, float* partial, long long npart, const int* rowb,
                                     const int* rowr, long long P, int n_group, int B, long long R, float c1, float c2,
                                     void* stream) {
    T2_REQUIRE(end_w || mix_w, "wg_head_bwd: neither a flow to close (end_w) nor one to open (mix_w)");
    T2_REQUIRE(rowb && rowr && x_sv && partial, "wg_head_bwd: null operand");
    T2_REQUIRE(P > 0 && B > 0 && R > 0, "wg_head_bwd: no rows");
    T2_REQUIRE(C > 0 && C <= WG_MAXC, "wg_head_bwd: C must be in 1..512");
    T2_REQUIRE(n_group >= 2 && n_group <= WG_MAXG && n_group % 2 == 0, "wg_head_bwd: n_group must be even and at most 16");
    if (end_w) {
        T2_REQUIRE(skip && log_s && a_in && dA && d_skip, "wg_head_bwd: null operand");
        T2_REQUIRE(n_in >= 2 && n_in % 2 == 0 && n_in <= n_group, "wg_head_bwd: n_in must be even and at most n_group");
        T2_REQUIRE(ldskip >= C && ldds >= C, "wg_head_bwd: skip rows too short");
        T2_REQUIRE(lsc >= R && lsb >= (long long)(n_in / 2) * lsc, "wg_head_bwd: bad log_s strides");
        T2_REQUIRE(ldain >= n_in && lddA >= n_in, "wg_head_bwd: audio rows too short");
    }
    const int n_cur = end_w ? n_in : n_group;
    T2_REQUIRE(n_emit >= 0 && n_emit % 2 == 0 && n_emit <= n_cur, "wg_head_bwd: n_emit must be even and at most the channels held");
    T2_REQUIRE(ldx >= n_cur, "wg_head_bwd: saved rows too short");
    const int n_out = n_cur - n_emit;
    long long want = 0;
    if (end_w) want += (long long)n_in * C + n_in;
    if (mix_w) {
        T2_REQUIRE(n_out >= 2, "wg_head_bwd: the next flow needs at least 2 channels");
        T2_REQUIRE(start_w && dh0 && a_sv && dA, "wg_head_bwd: the next flow needs start_w, dh0, its saved rows and dA");
        T2_REQUIRE(lddh >= C && ldasv >= n_out / 2 && lddA >= n_out, "wg_head_bwd: rows of the next flow too short");
        want += (long long)C * (n_out / 2) + C + (long long)n_out * n_out;
    } else {
        T2_REQUIRE(n_out == 0, "wg_head_bwd: the last call emitted every remaining channel");
        T2_REQUIRE(!start_w, "wg_head_bwd: the last flow has no next start");
    }
    T2_REQUIRE(npart == want, "wg_head_bwd: npart must be the number of small gradients of this call");
    const long long nblk = (P + WGB_ROWS * WGB_SUB - 1) / (WGB_ROWS * WGB_SUB);
    T2_REQUIRE(nblk <= 0x7fffffffLL, "wg_head_bwd: too many rows");
    T2_LAUNCH(wg_head_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, skip, ldskip, C, end_w, n_in, log_s,
              lsb, lsc, a_in, ldain, x_sv, ldx, a_sv, ldasv, dA, lddA, dh0, lddh, mix_w, start_w, n_emit, d_skip, ldds, partial,
              npart, rowb, rowr, P, n_group, B, R, c1, c2);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// out[i] = sum over blk < nblk, in that order, of partial[blk * n + i].
__global__ void __launch_bounds__(256) wg_partial_sum_kernel(const float* __restrict__ partial, long long nblk, long long n,
                                                             float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (long long blk = 0; blk < nblk; ++blk) s += partial[blk * n + i];
    out[i] = s;
}

extern "C" int t2amd_wg_partial_sum_f32(const float* partial, long long nblk, long long n, float* out, void* stream) {
    T2_REQUIRE(partial && out, "wg_partial_sum: null operand");
    T2_REQUIRE(nblk > 0 && n > 0 && (n + 255) / 256 <= 0x7fffffffLL, "wg_partial_sum: bad dims");
    T2_LAUNCH(wg_partial_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, partial, nblk, n, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// Gate backward, acts = tanh(u) sigmoid(v) with the saved gate values gate[m] = [t = tanh(u) (C) | s = sigmoid(v) (C)]: for
// every row m with rowb[m] >= 0
//   d_pre[m][c] = d_acts[m][c] s (1 - t^2),  d_pre[m][C + c] = d_acts[m][c] t s (1 - s),  acts[m][c] = t s
// (d_pre in the order of the cond slab and of the in-layer bias: tanh channels, then sigmoid channels; acts is what the
// residual / skip weight gradient multiplies).  Other rows are not written: they stay zero.
__global__ void __launch_bounds__(256) wg_gate_bwd_kernel(const float* __restrict__ d_acts, long long ldd,
                                                          const float* __restrict__ gate, long long ldg,
                                                          const int* __restrict__ rowb, long long M, int C,
                                                          float* __restrict__ d_pre, long long ldp, float* __restrict__ acts,
                                                          long long lda) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const long long m = i / C;
    const int c = (int)(i - m * C);
    if (rowb[m] < 0) return;
    const float g = d_acts[m * ldd + c];
    const float t = gate[m * ldg + c], s = gate[m * ldg + C + c];
    d_pre[m * ldp + c] = g * s * (1.0f - t * t);
    d_pre[m * ldp + C + c] = g * t * (s * (1.0f - s));
    acts[m * lda + c] = t * s;
}

extern "C" int t2amd_wg_gate_bwd_f32(const float* d_acts, long long ldd, const float* gate, long long ldg, const int* rowb,
                                     long long M, int C, float* d_pre, long long ldp, float* acts, long long lda, void* stream) {
    T2_REQUIRE(d_acts && gate && rowb && d_pre && acts, "wg_gate_bwd: null operand");
    T2_REQUIRE(M > 0 && C > 0 && C <= WG_MAXC, "wg_gate_bwd: bad dims");
    T2_REQUIRE(ldd >= C && lda >= C && ldg >= 2 * C && ldp >= 2 * C, "wg_gate_bwd: rows too short");
    const long long nblk = (M * C + 255) / 256;
    T2_REQUIRE(nblk <= 0x7fffffffLL, "wg_gate_bwd: too many rows");
    T2_LAUNCH(wg_gate_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, d_acts, ldd, gate, ldg, rowb, M, C,
              d_pre, ldp, acts, lda);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
