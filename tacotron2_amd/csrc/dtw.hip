// Mel-cepstral distortion under dynamic time warping (tacotron2_amd/audio.py MelCepstralDistortion).
//   mel_cepstrum:  c[b][t][k-1] = sum_m basis[k-1][m] mel[b][m][t], ascending m, one fma each; basis (K, n_mel) is the orthonormal
//                  DCT-II without c0, built on the host in float64 and rounded once.  Rows at and beyond lengths[b] are zeros.
//   dtw:           one workgroup per pair.  d(i,j) = sqrt(sum_k (a_ik - b_jk)^2), differences first;
//                  D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)), D(0,0) = d(0,0), absent predecessors are +inf.
//                  Ties: the diagonal, then (i-1,j), then (i,j-1) (the strict `<` chain of dtw_cell).  Every accumulated cost
//                  carries the cell count of its path, so the path length needs no backtrack.
//   backtrack:     one lane per pair walks the predecessor bytes from (n_a-1, n_b-1) to (0,0) and writes (i, j) in forward order.
// Layout of dtw: lanes own the rows of a band of DTW_W rows; lane r at step s does column s - r, so a step is one anti-diagonal of
// the band.  What lane r needs from the row above is what lane r-1 published one step earlier (D(i-1,j)) and what it read itself
// one step earlier (D(i-1,j-1)): an LDS double buffer and one __syncthreads() per step.  D(i,j-1) is the lane's own register.  The
// last row of a full band goes to an LDS row buffer that lane 0 of the next band reads; its writer is DTW_W - 1 columns behind
// the reader, so the buffer is updated in place.  d(i,j) does not depend on the recurrence: the cell's distance for the NEXT
// step is computed before this step's LDS wait, which takes the loads of b out of the loop-carried chain.  a_i lives in
// registers; b is read through the cache (a wave reads 64 consecutive rows, shifted by one row per step).
// One writer per element, fixed order, no atomics: two calls give the same bits and a pair in a ragged batch gives the bits it
// gives alone.  Plain C++ and __syncthreads only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define DTW_W 256                       /* rows of a band = lanes of the workgroup */
#define DTW_MAX_LEN 4096                /* frames of one side, at most: the row buffer is 32 KiB of LDS */
#define DTW_MAX_K 32
#define CEP_THREADS 256
#define CEP_MAX_BASIS 8192              /* floats of the basis in LDS: K n_mel at most */
#define BT_THREADS 64

__global__ void __launch_bounds__(CEP_THREADS) mel_cepstrum_kernel(const float* __restrict__ mel, long long ldb, long long ldm,
                                                                   const int* __restrict__ lengths, int n_mel, int T,
                                                                   const float* __restrict__ basis, int K, float* __restrict__ out) {
    __shared__ float bs[CEP_MAX_BASIS];
    const int b = blockIdx.y, t = blockIdx.x * CEP_THREADS + threadIdx.x;
    for (int e = threadIdx.x; e < K * n_mel; e += CEP_THREADS) bs[e] = basis[e];
    __syncthreads();
    if (t >= T) return;
    const int len = lengths ? t2_clamp_count(lengths[b], T) : T;
    float acc[DTW_MAX_K];
#pragma unroll
    for (int k = 0; k < DTW_MAX_K; ++k) acc[k] = 0.0f;
    if (t < len) {
        const float* x = mel + b * ldb + t;
        for (int m = 0; m < n_mel; ++m) {
            const float v = x[m * ldm];
#pragma unroll
            for (int k = 0; k < DTW_MAX_K; ++k)
                if (k < K) acc[k] = fmaf(bs[k * n_mel + m], v, acc[k]);
        }
    }
    float* o = out + ((long long)b * T + t) * K;
#pragma unroll
    for (int k = 0; k < DTW_MAX_K; ++k)
        if (k < K) o[k] = acc[k];
}

// sqrt(sum_k (a_k - b_k)^2): the difference first, ascending k, one fma each.
__device__ __forceinline__ float dtw_dist(const float (&ar)[DTW_MAX_K], const float* __restrict__ bj, int K) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < DTW_MAX_K; ++k)
        if (k < K) {
            const float df = ar[k] - bj[k];
            acc = fmaf(df, df, acc);
        }
    return sqrtf(acc);
}

__global__ void __launch_bounds__(DTW_W) dtw_kernel(const float* __restrict__ a, long long sa, const float* __restrict__ b,
                                                    long long sb, const int* __restrict__ na, const int* __restrict__ nb, int Ta,
                                                    int Tb, int K, float* __restrict__ cost, int* __restrict__ steps,
                                                    unsigned char* __restrict__ path, int path_rows, int path_cols) {
    __shared__ float rowc[DTW_MAX_LEN];
    __shared__ int rown[DTW_MAX_LEN];
    __shared__ float hc[2][DTW_W];
    __shared__ int hn[2][DTW_W];
    const int p = blockIdx.x, r = threadIdx.x;
    int cap_a = Ta < DTW_MAX_LEN ? Ta : DTW_MAX_LEN, cap_b = Tb < DTW_MAX_LEN ? Tb : DTW_MAX_LEN;
    if (path) {                                                             // never write outside the caller's slab
        cap_a = cap_a < path_rows ? cap_a : path_rows;
        cap_b = cap_b < path_cols ? cap_b : path_cols;
    }
    const int n_a = na ? t2_clamp_count(na[p], cap_a) : cap_a;
    const int n_b = nb ? t2_clamp_count(nb[p], cap_b) : cap_b;
    if (n_a < 1 || n_b < 1) {                                               // uniform; the host refuses such lengths
        if (r == 0) {
            cost[p] = 0.0f;
            steps[p] = 0;
        }
        return;
    }
    a += p * sa;
    b += p * sb;
    if (path) path += (long long)p * path_rows * path_cols;
    const float inf = __uint_as_float(0x7f800000u);
    for (int i0 = 0; i0 < n_a; i0 += DTW_W) {
        const int rows = n_a - i0 < DTW_W ? n_a - i0 : DTW_W;
        const bool feeds_next = i0 + DTW_W < n_a;                           // then the band is full and lane DTW_W - 1 owns its last row
        const int i = i0 + r;
        const bool active = r < rows;
        float ar[DTW_MAX_K];
#pragma unroll
        for (int k = 0; k < DTW_MAX_K; ++k) ar[k] = active && k < K ? a[(long long)i * K + k] : 0.0f;
        float left_c = inf, diag_c = inf;
        int left_n = 0, diag_n = 0;
        const int nsteps = n_b + rows - 1;
        float d_cur = active && r == 0 ? dtw_dist(ar, b, K) : 0.0f;         // step 0: only lane 0 has a column
        for (int s = 0; s < nsteps; ++s) {
            const int j = s - r, jn = j + 1;
            float d_next = 0.0f;
            if (active && jn >= 0 && jn < n_b) d_next = dtw_dist(ar, b + (long long)jn * K, K);
            if (active && j >= 0 && j < n_b) {
                float up_c = inf;
                int up_n = 0;
                if (r > 0) {
                    up_c = hc[(s + 1) & 1][r - 1];
                    up_n = hn[(s + 1) & 1][r - 1];
                } else if (i0 > 0) {
                    up_c = rowc[j];
                    up_n = rown[j];
                }
                if (j == 0) diag_c = inf;                                   // (left_c is still +inf there)
                // the tie rule: the diagonal, then (i-1, j), then (i, j-1)
                float best_c = diag_c;
                int best_n = diag_n, ch = 0;
                if (up_c < best_c) {
                    best_c = up_c;
                    best_n = up_n;
                    ch = 1;
                }
                if (left_c < best_c) {
                    best_c = left_c;
                    best_n = left_n;
                    ch = 2;
                }
                const bool origin = i == 0 && j == 0;
                const float c = origin ? d_cur : d_cur + best_c;
                const int n = origin ? 1 : best_n + 1;
                hc[s & 1][r] = c;
                hn[s & 1][r] = n;
                if (feeds_next && r == DTW_W - 1) {
                    rowc[j] = c;
                    rown[j] = n;
                }
                if (path) path[(long long)i * path_cols + j] = (unsigned char)ch;
                if (i == n_a - 1 && j == n_b - 1) {
                    cost[p] = c;
                    steps[p] = n;
                }
                left_c = c;
                left_n = n;
                diag_c = up_c;
                diag_n = up_n;
            }
            d_cur = d_next;
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(BT_THREADS) dtw_backtrack_kernel(const unsigned char* __restrict__ path, int path_rows,
                                                                   int path_cols, const int* __restrict__ na,
                                                                   const int* __restrict__ nb, const int* __restrict__ steps, int B,
                                                                   int Ta, int Tb, int* __restrict__ out, int L) {
    const int p = blockIdx.x * BT_THREADS + threadIdx.x;
    if (p >= B) return;
    int cap_a = Ta < DTW_MAX_LEN ? Ta : DTW_MAX_LEN, cap_b = Tb < DTW_MAX_LEN ? Tb : DTW_MAX_LEN;
    cap_a = cap_a < path_rows ? cap_a : path_rows;
    cap_b = cap_b < path_cols ? cap_b : path_cols;
    const int n_a = na ? t2_clamp_count(na[p], cap_a) : cap_a;
    const int n_b = nb ? t2_clamp_count(nb[p], cap_b) : cap_b;
    path += (long long)p * path_rows * path_cols;
    out += (long long)p * L * 2;
    int len = n_a < 1 || n_b < 1 ? 0 : steps[p];
    len = len < 0 ? 0 : (len > L ? L : len);
    for (int e = len; e < L; ++e) {
        out[2 * e] = -1;
        out[2 * e + 1] = -1;
    }
    int i = n_a - 1, j = n_b - 1, e = len - 1;
    for (; e >= 0; --e) {
        out[2 * e] = i;
        out[2 * e + 1] = j;
        if (i == 0 && j == 0) break;
        int ch = path[(long long)i * path_cols + j];
        if (i == 0) ch = 2;                                                 // whatever the byte says, the walk stays inside
        else if (j == 0) ch = 1;
        if (ch != 2) --i;
        if (ch != 1) --j;
    }
    for (--e; e >= 0; --e) {                                                // a count longer than the walk: never with dtw's own
        out[2 * e] = -1;
        out[2 * e + 1] = -1;
    }
}

extern "C" int t2amd_dtw_width(void) { return DTW_W; }

extern "C" int t2amd_mel_cepstrum_f32(const float* mel, long long ldb, long long ldm, const int* lengths, int B, int n_mel, int T,
                                      const float* basis, int K, float* out, void* stream) {
    T2_REQUIRE(mel && basis && out, "mel_cepstrum: null operand");
    T2_REQUIRE(K >= 1 && K <= DTW_MAX_K, "mel_cepstrum: 1 to 32 coefficients");
    T2_REQUIRE(B >= 1 && B <= 65535 && n_mel >= 1 && T >= 1 && T <= 16777216, "mel_cepstrum: bad shape");
    T2_REQUIRE((long long)K * n_mel <= CEP_MAX_BASIS, "mel_cepstrum: the basis holds more than 8192 floats (n_coef x n_mel)");
    T2_REQUIRE(ldm >= T && ldb >= (n_mel - 1) * ldm + T, "mel_cepstrum: row too short");
    const long long ob = 4LL * B * T * K, mb = 4 * ((B - 1) * ldb + (n_mel - 1) * ldm + T);
    T2_REQUIRE(!t2_overlap(out, ob, mel, mb) && !t2_overlap(out, ob, basis, 4LL * K * n_mel) &&
                   !(lengths && t2_overlap(out, ob, lengths, 4LL * B)),
               "mel_cepstrum: out must not be one of the inputs");
    T2_LAUNCH(mel_cepstrum_kernel, dim3((unsigned)((T + CEP_THREADS - 1) / CEP_THREADS), (unsigned)B), dim3(CEP_THREADS), 0,
              (hipStream_t)stream, mel, ldb, ldm, lengths, n_mel, T, basis, K, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

static int dtw_check(const char* who, int B, int Ta, int Tb, const void* na, const void* nb, bool slab, int path_rows, int path_cols,
                     char* msg) {
    const char* what = !(B >= 1 && B <= 1048576)                             ? "1 to 2^20 pairs"
                       : !(Ta >= 1 && Tb >= 1)                               ? "sequences of at least 1 frame"
                       : !((na || Ta <= DTW_MAX_LEN) && (nb || Tb <= DTW_MAX_LEN)) ? "sequences of at most 4096 frames"
                       : slab && !(path_rows >= 1 && path_cols >= 1 && path_rows <= DTW_MAX_LEN && path_cols <= DTW_MAX_LEN)
                           ? "a predecessor slab of 1 to 4096 rows and columns"
                           : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, 160, "%s: %s", who, what);
    return T2AMD_ERR_ARG;
}

extern "C" int t2amd_dtw_f32(const float* a, long long sa, const float* b, long long sb, const int* na, const int* nb, int B, int Ta,
                             int Tb, int K, float* cost, int* steps, unsigned char* path, int path_rows, int path_cols,
                             void* stream) {
    char msg[160];
    T2_REQUIRE(a && b && cost && steps, "dtw: null operand");
    T2_REQUIRE(K >= 1 && K <= DTW_MAX_K, "dtw: 1 to 32 coefficients");
    if (dtw_check("dtw", B, Ta, Tb, na, nb, path != nullptr, path_rows, path_cols, msg) != T2AMD_OK) T2_FAIL(msg);
    T2_REQUIRE(sa >= (long long)Ta * K && sb >= (long long)Tb * K, "dtw: pair stride too short");
    T2_REQUIRE(!path || (na && nb) || (path_rows >= (Ta < DTW_MAX_LEN ? Ta : DTW_MAX_LEN) && path_cols >= (Tb < DTW_MAX_LEN ? Tb : DTW_MAX_LEN)),
               "dtw: the predecessor slab is smaller than the sequences");
    T2_LAUNCH(dtw_kernel, dim3((unsigned)B), dim3(DTW_W), 0, (hipStream_t)stream, a, sa, b, sb, na, nb, Ta, Tb, K, cost, steps, path,
              path_rows, path_cols);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_dtw_backtrack(const unsigned char* path, int path_rows, int path_cols, const int* na, const int* nb,
                                   const int* steps, int B, int Ta, int Tb, int* out, int L, void* stream) {
    char msg[160];
    T2_REQUIRE(path && steps && out, "dtw_backtrack: null operand");
    if (dtw_check("dtw_backtrack", B, Ta, Tb, na, nb, true, path_rows, path_cols, msg) != T2AMD_OK) T2_FAIL(msg);
    T2_REQUIRE(L >= 1 && L <= 2 * DTW_MAX_LEN - 1, "dtw_backtrack: a path of 1 to 8191 cells");
    T2_LAUNCH(dtw_backtrack_kernel, dim3((unsigned)((B + BT_THREADS - 1) / BT_THREADS)), dim3(BT_THREADS), 0, (hipStream_t)stream,
              path, path_rows, path_cols, na, nb, steps, B, Ta, Tb, out, L);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
