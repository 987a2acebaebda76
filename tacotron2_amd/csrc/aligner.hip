// Learned-aligner scores, the three products (tacotron2_amd/alignment.py), on the MFMA tile loop of
// csrc/rowmma.h: rm_tile_f32 clients (v_mfma_f32_32x32x2_f32, exact f32, every sum over the reduction index ascending) with their
// own Rows policies and __global__ wrappers, 128 x 64 tiles (2 x 2 waves of 2 x 1 MFMA tiles), blockIdx.z = utterance.
//   1. z[t][n]  = tau (2 sum_c q[t][c] k[n][c] - |k_n|^2)          A = query rows (zero-filled beyond C in the policy),
//                                                                  B = the key slab Kp [N][Cp]; reduction over Cp.
//   2. dQ[t][c] = 2 tau sum_n dz[t][n] k[n][c]                     A = dz rows [T][Np], B = KT [C][Np]; reduction over Np.
//   3. dK[n][c] = 2 tau (sum_t dz[t][n] q[t][c] - cs[n] k[n][c])   A = dz read down its columns (a strided policy, zero at
//                                                                  and beyond T_b), B = QT [C][Tp]; reduction over Tp.
// The reduction lengths are the batch's own, rounded up to 32; what lies beyond an utterance's count is zero in both operands,
// and adding +0 to a sum that started at +0 changes no bit, so an utterance in a ragged batch gives the bits it gives alone.
// Products 2 and 3 write the exact zeros of the padding themselves (one writer per element): a tile wholly beyond the
// utterance's rows stores zeros and leaves before the loop.  The slabs, the row passes between the products and the prior are in
// csrc/aligner_rows.hip; csrc/aligner.h holds the layouts.
#include "aligner.h"
#include "rowmma.h"

#define AL_BN 64

struct AlProd {
    const float* A;                     // product 1: q (B, T_max, C); 2 and 3: dz (B, T_max, Np)
    const float* W;                     // the B operand slab, [rows][K] per utterance, wb floats an utterance
    long long wb;
    float* out;                         // 1: z at (ob, ldo); 2: dQ (B, T_max, C); 3: dK (B, N_max, C)
    long long ob, ldo;
    const float* aux;                   // 1: |k_n|^2 (B, N_max); 3: the column sums of dz (B, N_max)
    const float* Kp;                    // 3: the key slab (B, N_max, Cp)
    const int* t_len;
    const int* n_len;
    int T_max, N_max, C, Cp, Np, K;
    float scale;                        // 1: tau; 2 and 3: 2 tau
};

// row of element r of a 32 x 32 accumulator tile, and its column, as csrc/rowmma.h states them
#define AL_FOR_TILE(TM, TN, body)                                                                                          \
    _Pragma("unroll") for (int tn = 0; tn < TN; ++tn) {                                                                    \
        const int gn = col0 + (wn * TN + tn) * 32 + (lane & 31);                                                           \
        _Pragma("unroll") for (int tm = 0; tm < TM; ++tm) _Pragma("unroll") for (int r = 0; r < 16; ++r) {                 \
            const int gm = row0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);                          \
            const float v = acc[tm][tn][r];                                                                                \
            body                                                                                                           \
        }                                                                                                                  \
    }

struct AlScoreRows {
    const float* q;                     // the utterance's queries [T][C]
    int C, T, N, row0, col0;
    float* out;
    long long ldo;
    const float* kn;
    float tau;
    bool vec;                           // C is a multiple of 4 and the utterance starts on 16 bytes: every row does
    __device__ __forceinline__ RmStep step(int k0) const { return {0, k0}; }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const int t = row0 + r, c = s.col + kc;
        if (t >= T || c >= C) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float* p = q + (long long)t * C + c;
        if (vec) return *reinterpret_cast<const float4*>(p);               // c + 3 < C
        return make_float4(p[0], c + 1 < C ? p[1] : 0.f, c + 2 < C ? p[2] : 0.f, c + 3 < C ? p[3] : 0.f);
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        AL_FOR_TILE(TM, TN, if (gm < T && gn < N) out[gm * ldo + gn] = tau * (2.0f * v - kn[gn]);)
    }
};

struct AlDqRows {
    const float* dz;                    // the utterance's dz [T_max][Np]
    int Np, T, T_max, C, row0, col0;
    float* out;                         // [T_max][C]
    float scale;
    __device__ __forceinline__ RmStep step(int k0) const { return {0, k0}; }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const int t = row0 + r;
        return t < T ? *reinterpret_cast<const float4*>(dz + (long long)t * Np + s.col + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        AL_FOR_TILE(TM, TN, if (gm < T_max && gn < C) out[(long long)gm * C + gn] = gm < T ? scale * v : 0.0f;)
    }
};

struct AlDkRows {
    const float* dz;                    // read down its columns: tile row = token, reduction index = frame
    int Np, T, N, N_max, C, Cp, row0, col0;
    float* out;                         // [N_max][C]
    const float* cs;
    const float* Kp;
    float scale;
    __device__ __forceinline__ RmStep step(int k0) const { return {0, k0}; }
    __device__ __forceinline__ float at(int t, int n) const { return t < T ? dz[(long long)t * Np + n] : 0.f; }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const int n = row0 + r, t = s.col + kc;
        if (n >= N) return make_float4(0.f, 0.f, 0.f, 0.f);
        return make_float4(at(t, n), at(t + 1, n), at(t + 2, n), at(t + 3, n));
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        AL_FOR_TILE(TM, TN, if (gm < N_max && gn < C) out[(long long)gm * C + gn] =
                                gm < N ? scale * fmaf(-cs[gm], Kp[(long long)gm * Cp + gn], v) : 0.0f;)
    }
};

// zeros on the rows row0 .. row0 + 127 below `rows` and the columns col0 .. col0 + 63 below C of out [rows][C]
__device__ __forceinline__ void al_zero_tile(float* out, int rows, int C, int row0, int col0) {
    for (int i = threadIdx.x; i < 128 * AL_BN; i += 256) {
        const int gm = row0 + i / AL_BN, gn = col0 + i % AL_BN;
        if (gm < rows && gn < C) out[(long long)gm * C + gn] = 0.0f;
    }
}

// blockIdx.x = row tile, blockIdx.y = column tile, blockIdx.z = utterance
__global__ __launch_bounds__(256) void aligner_z_kernel(AlProd p) {
    const int b = blockIdx.z, row0 = blockIdx.x * 128, col0 = blockIdx.y * AL_BN;
    const int T = t2_clamp_count(p.t_len[b], p.T_max), N = t2_clamp_count(p.n_len[b], p.N_max);
    if (row0 >= T || col0 >= N) return;                                     // uniform: the row pass writes the padding
    const float* q = p.A + (long long)b * p.T_max * p.C;
    const AlScoreRows rows{q, p.C, T, N, row0, col0, p.out + b * p.ob, p.ldo, p.aux + (long long)b * p.N_max, p.scale,
                           (p.C & 3) == 0 && (reinterpret_cast<uintptr_t>(q) & 15u) == 0};
    rm_tile_f32<2, 2, 2, 1>(rows, p.W + b * p.wb, N, p.K, col0);
}

__global__ __launch_bounds__(256) void aligner_dq_kernel(AlProd p) {
    const int b = blockIdx.z, row0 = blockIdx.x * 128, col0 = blockIdx.y * AL_BN;
    const int T = t2_clamp_count(p.t_len[b], p.T_max);
    float* out = p.out + (long long)b * p.T_max * p.C;
    if (row0 >= T) {                                                        // uniform
        al_zero_tile(out, p.T_max, p.C, row0, col0);
        return;
    }
    const AlDqRows rows{p.A + (long long)b * p.T_max * p.Np, p.Np, T, p.T_max, p.C, row0, col0, out, p.scale};
    rm_tile_f32<2, 2, 2, 1>(rows, p.W + b * p.wb, p.C, p.K, col0);
}

__global__ __launch_bounds__(256) void aligner_dk_kernel(AlProd p) {
    const int b = blockIdx.z, row0 = blockIdx.x * 128, col0 = blockIdx.y * AL_BN;
    const int T = t2_clamp_count(p.t_len[b], p.T_max), N = t2_clamp_count(p.n_len[b], p.N_max);
    float* out = p.out + (long long)b * p.N_max * p.C;
    if (row0 >= N) {                                                        // uniform
        al_zero_tile(out, p.N_max, p.C, row0, col0);
        return;
    }
    const AlDkRows rows{p.A + (long long)b * p.T_max * p.Np, p.Np, T, N, p.N_max, p.C, p.Cp, row0, col0, out,
                        p.aux + (long long)b * p.N_max, p.Kp + (long long)b * p.N_max * p.Cp, p.scale};
    rm_tile_f32<2, 2, 2, 1>(rows, p.W + b * p.wb, p.C, p.K, col0);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static int al_common(const char* who, const float* q, const float* k, const int* t_len, const int* n_len, int B, int T_max,
                     int N_max, int C, float tau, const unsigned char* ws, long long ws_bytes, long long need) {
    char msg[160];
    const char* what = !(q && k && t_len && n_len && ws)      ? "null operand"
                       : !(tau > 0.0f && tau <= 3.0e38f)      ? "the temperature must be positive and finite"
                       : !(ws_bytes >= need)                  ? "the workspace is smaller than t2amd_aligner_workspace asks for"
                       : !t2_aligned16(ws)                    ? "the workspace is not aligned to 16 bytes"
                                                              : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    T2_FAIL(msg);
}

static void al_launch_z(const AlProd& p, int B, hipStream_t s) {
    T2_LAUNCH(aligner_z_kernel, dim3((unsigned)t2_cdiv(p.T_max, 128), (unsigned)t2_cdiv(p.N_max, AL_BN), (unsigned)B), dim3(256), 0, s, p);
}

extern "C" int t2amd_aligner_scores_f32(const float* q, const float* k, const int* t_len, const int* n_len, int B, int T_max,
                                        int N_max, int C, float tau, const float* logp, long long pb, long long pt, float* scores,
                                        long long sb, long long st, int keep, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(al_check("aligner_scores", B, T_max, N_max, C));
    const AlFwdWs w = al_fwd_ws(B, T_max, N_max, C, keep);
    T2_PROPAGATE(al_common("aligner_scores", q, k, t_len, n_len, B, T_max, N_max, C, tau, ws, ws_bytes, w.bytes));
    T2_REQUIRE(scores, "aligner_scores: null operand");
    T2_REQUIRE(t2_strides_cover(sb, st, B, T_max, N_max), "aligner_scores: score strides shorter than the matrix");
    const long long sbytes = t2_span_bytes(sb, st, B, T_max, N_max);
    T2_REQUIRE(!t2_overlap(scores, sbytes, q, 4LL * B * T_max * C) && !t2_overlap(scores, sbytes, k, 4LL * B * N_max * C) &&
                   !t2_overlap(scores, sbytes, ws, ws_bytes),
               "aligner_scores: the scores must not overlap the inputs or the workspace");
    float* Kp = reinterpret_cast<float*>(ws + w.kp);
    float* kn = reinterpret_cast<float*>(ws + w.kn);
    T2_PROPAGATE(t2amd_aligner_pack_keys_f32(k, n_len, B, N_max, C, Kp, kn, stream));
    AlProd p = {};
    p.A = q; p.W = Kp; p.wb = (long long)N_max * w.Cp; p.out = scores; p.ob = sb; p.ldo = st; p.aux = kn;
    p.t_len = t_len; p.n_len = n_len; p.T_max = T_max; p.N_max = N_max; p.C = C; p.Cp = w.Cp; p.K = w.Cp; p.scale = tau;
    al_launch_z(p, B, (hipStream_t)stream);
    T2_LAUNCH_CHECK();
    return t2amd_aligner_rows_fwd_f32(scores, sb, st, logp, pb, pt, t_len, n_len, B, T_max, N_max,
                                      keep ? reinterpret_cast<float*>(ws + w.lse) : nullptr, stream);
}

// one product of the backward alone, on the slabs of t2amd_aligner_scores_bwd_f32's workspace
extern "C" int t2amd_aligner_product_f32(int which, const float* q, const float* k, const int* t_len, const int* n_len, int B,
                                         int T_max, int N_max, int C, float tau, float* dq, float* dk, const unsigned char* kept,
                                         long long kept_bytes, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(al_check("aligner_product", B, T_max, N_max, C));
    const AlFwdWs f = al_fwd_ws(B, T_max, N_max, C, 1);
    const AlBwdWs w = al_bwd_ws(B, T_max, N_max, C);
    T2_PROPAGATE(al_common("aligner_product", q, k, t_len, n_len, B, T_max, N_max, C, tau, ws, ws_bytes, w.bytes));
    T2_REQUIRE(which >= 1 && which <= 3, "aligner_product: which must be 1 (z), 2 (dQ) or 3 (dK)");
    T2_REQUIRE(kept && (which != 2 || dq) && (which != 3 || dk), "aligner_product: null operand");
    T2_REQUIRE(kept_bytes >= f.bytes && t2_aligned16(kept),
               "aligner_product: the kept workspace is not what t2amd_aligner_scores_f32 left with keep != 0");
    float* dz = reinterpret_cast<float*>(ws + w.dz);
    const float* Kp = reinterpret_cast<const float*>(kept + f.kp);
    hipStream_t s = (hipStream_t)stream;
    AlProd p = {};
    p.t_len = t_len; p.n_len = n_len; p.T_max = T_max; p.N_max = N_max; p.C = C; p.Cp = f.Cp; p.Np = w.Np;
    if (which == 1) {                                                       // z again, into the dz slab
        p.A = q; p.W = Kp; p.wb = (long long)N_max * f.Cp; p.out = dz; p.ob = (long long)T_max * w.Np; p.ldo = w.Np;
        p.aux = reinterpret_cast<const float*>(kept + f.kn); p.K = f.Cp; p.scale = tau;
        T2_LAUNCH(aligner_z_kernel, dim3((unsigned)t2_cdiv(T_max, 128), (unsigned)t2_cdiv(N_max, AL_BN), (unsigned)B), dim3(256), 0, s, p);
    } else if (which == 2) {
        p.A = dz; p.W = reinterpret_cast<const float*>(ws + w.kt); p.wb = (long long)C * w.Np; p.out = dq; p.K = w.Np;
        p.scale = 2.0f * tau;
        T2_LAUNCH(aligner_dq_kernel, dim3((unsigned)t2_cdiv(T_max, 128), (unsigned)t2_cdiv(C, AL_BN), (unsigned)B), dim3(256), 0, s, p);
    } else {
        p.A = dz; p.W = reinterpret_cast<const float*>(ws + w.qt); p.wb = (long long)C * w.Tp; p.out = dk; p.K = w.Tp;
        p.aux = reinterpret_cast<const float*>(ws + w.cs); p.Kp = Kp; p.scale = 2.0f * tau;
        T2_LAUNCH(aligner_dk_kernel, dim3((unsigned)t2_cdiv(N_max, 128), (unsigned)t2_cdiv(C, AL_BN), (unsigned)B), dim3(256), 0, s, p);
    }
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_aligner_scores_bwd_f32(const float* q, const float* k, const int* t_len, const int* n_len, int B, int T_max,
                                            int N_max, int C, float tau, const float* g, long long gb, long long gt, float* dq,
                                            float* dk, float* dlogp, long long db, long long dt, const unsigned char* kept,
                                            long long kept_bytes, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(al_check("aligner_scores_bwd", B, T_max, N_max, C));
    const AlFwdWs f = al_fwd_ws(B, T_max, N_max, C, 1);
    const AlBwdWs w = al_bwd_ws(B, T_max, N_max, C);
    T2_PROPAGATE(al_common("aligner_scores_bwd", q, k, t_len, n_len, B, T_max, N_max, C, tau, ws, ws_bytes, w.bytes));
    T2_REQUIRE(g && dq && dk && kept, "aligner_scores_bwd: null operand");
    T2_REQUIRE(kept_bytes >= f.bytes && t2_aligned16(kept),
               "aligner_scores_bwd: the kept workspace is not what t2amd_aligner_scores_f32 left with keep != 0");
    const long long qbytes = 4LL * B * T_max * C, kbytes = 4LL * B * N_max * C;
    T2_REQUIRE(!t2_overlap(dq, qbytes, q, qbytes) && !t2_overlap(dq, qbytes, k, kbytes) && !t2_overlap(dk, kbytes, q, qbytes) &&
                   !t2_overlap(dk, kbytes, k, kbytes) && !t2_overlap(dq, qbytes, dk, kbytes) && !t2_overlap(dq, qbytes, ws, ws_bytes) &&
                   !t2_overlap(dk, kbytes, ws, ws_bytes) && !t2_overlap(ws, ws_bytes, kept, kept_bytes) &&
                   !t2_overlap(dq, qbytes, kept, kept_bytes) && !t2_overlap(dk, kbytes, kept, kept_bytes),
               "aligner_scores_bwd: outputs and workspace must not overlap the inputs or each other");
    const float* lse = reinterpret_cast<const float*>(kept + f.lse);
    float* dz = reinterpret_cast<float*>(ws + w.dz);
    T2_PROPAGATE(t2amd_aligner_product_f32(1, q, k, t_len, n_len, B, T_max, N_max, C, tau, dq, dk, kept, kept_bytes, ws, ws_bytes, stream));
    T2_PROPAGATE(t2amd_aligner_rows_bwd_f32(g, gb, gt, t_len, n_len, B, T_max, N_max, lse, dz, reinterpret_cast<float*>(ws + w.cs), dlogp,
                                            db, dt, stream));
    T2_PROPAGATE(t2amd_aligner_transpose_f32(k, n_len, B, N_max, C, reinterpret_cast<float*>(ws + w.kt), stream));
    T2_PROPAGATE(t2amd_aligner_transpose_f32(q, t_len, B, T_max, C, reinterpret_cast<float*>(ws + w.qt), stream));
    T2_PROPAGATE(t2amd_aligner_product_f32(2, q, k, t_len, n_len, B, T_max, N_max, C, tau, dq, dk, kept, kept_bytes, ws, ws_bytes, stream));
    return t2amd_aligner_product_f32(3, q, k, t_len, n_len, B, T_max, N_max, C, tau, dq, dk, kept, kept_bytes, ws, ws_bytes, stream);
}
