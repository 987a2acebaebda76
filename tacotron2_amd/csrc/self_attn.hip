// Masked multi-head self-attention, the MFMA kernels (tacotron2_amd/transformer.py): o = softmax(scale q k^T) v
// over each utterance's own frames, and its gradient, on v_mfma_f32_32x32x2_f32 (exact f32: every product a k-ordered fmaf chain).
// No (T, T) matrix exists in memory: the forward keeps a running maximum and sum per row, the backward recomputes the
// probabilities from the kept logsumexp.  The operand and accumulator layouts and the k-major LDS images are those of
// csrc/rowmma.h; the loop is this file's own, because three products hang together inside one step.
//
// Every product is written transposed, so that the row a lane cares about sits ON the lane.  An accumulator tile has its column on
// the lane (lane & 31) and its 16 rows in the registers, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) for register r.  With
//   forward      S^T = K Q^T (column = query),  O^T += V^T P^T
//   dK, dV       S = Q K^T, dP = g V^T (column = key),  dV^T += g^T P,  dK^T += Q^T dS
//   dQ           S^T, dP^T = V g^T (column = query),  dQ^T += K^T dS^T
// a row's maximum, sum, lse and delta are one scalar per lane (the two lanes l and l + 32 share a row and meet in one
// __shfl_xor), and the accumulator of the first product is already the B operand of the second: register r is reduction step r.
// For that step to carry the rows 2 r and 2 r + 1 of the tile, ascending, the k-major image puts row i of a group of 32 into
// MFMA slot sa_slot(i).  So every sum runs over its index ascending: d for the scores, the key j for o and dq, the query t for
// dk and dv.  The row sum of the forward is kept per lane (the keys of the lane's parity, ascending) and the two halves are
// added once at the end.
//
// A workgroup is 256 lanes = 4 waves of 32 rows (queries in the forward and in dQ, keys in dK/dV) and walks the other axis in
// steps of 64 (forward) or 32 (backward) up to the utterance's own length, never the batch's: an utterance in a ragged batch
// gives the bits it gives alone.  Rows at and beyond the length are never read; they are zero operands, and their outputs are
// written as +0 by the lane that owns them (one writer per element).  grid = (ceil(T / 128), B H).
#include "self_attn.h"

// A product and a following sum stay two roundings unless fmaf is written: the backward's p = exp(scale s - lse) must see the
// rounded scale s that the forward's lse was made from (fused, a lone key's p came out as 1 + 4 ulp instead of 1).
#pragma clang fp contract(off)

struct SaArgs {
    SaOperand q, k, v, g;
    const float* o;                     // backward: what the forward wrote
    const float* lse;                   // backward: kept (B, H, T)
    const float* delta;                 // backward: (B, H, T) from self_attn_delta_kernel
    float* out;                         // forward: o (B, T, H, D)
    float* out_lse;                     // forward: (B, H, T) or null
    float *dq, *dk, *dv;                // backward: (B, T, H, D)
    const int* len;
    int T, H;
    float scale;
};

__device__ __forceinline__ float sa_ninf() { return __uint_as_float(0xff800000u); }

// the MFMA row (of 32) that holds row i of a tile, so that register r of lane half h is row 2 r + h
__device__ __forceinline__ int sa_slot(int i) { return ((i >> 1) & 3) + 8 * (i >> 3) + 4 * (i & 1); }

// the B operand of a product over d held in registers: f[kk] = row[2 kk + lhi]; zeros where the row does not exist
template <int D>
__device__ __forceinline__ void sa_frag(const float* row, bool live, int lhi, float (&f)[D / 2]) {
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) v = t2_ld4(row + 4 * c);
        f[2 * c] = lhi ? v.y : v.x;
        f[2 * c + 1] = lhi ? v.w : v.z;
    }
}

// rows r0 .. r0 + ROWS - 1 of x (row stride st) as a k-major image img[d][ROWS + 1], row i of each group of 32 in slot sa_slot(i);
// zeros at and beyond T
template <int D, int ROWS>
__device__ __forceinline__ void sa_stage_kmajor(float* img, const float* x, long long st, int r0, int T) {
    constexpr int LD = ROWS + 1, Q4 = D / 4;
#pragma unroll
    for (int i = 0; i < ROWS * Q4 / 256; ++i) {
        const int f = threadIdx.x + 256 * i, rr = f / Q4, kq = f % Q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + rr < T) v = t2_ld4(x + (long long)(r0 + rr) * st + 4 * kq);
        float* p = img + (4 * kq) * LD + (rr & ~31) + sa_slot(rr & 31);
        p[0] = v.x;
        p[LD] = v.y;
        p[2 * LD] = v.z;
        p[3 * LD] = v.w;
    }
}

// the same rows as they lie, img[row][D + 4]
template <int D, int ROWS>
__device__ __forceinline__ void sa_stage_rows(float* img, const float* x, long long st, int r0, int T) {
    constexpr int LD = D + 4, Q4 = D / 4;
#pragma unroll
    for (int i = 0; i < ROWS * Q4 / 256; ++i) {
        const int f = threadIdx.x + 256 * i, rr = f / Q4, kq = f % Q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + rr < T) v = t2_ld4(x + (long long)(r0 + rr) * st + 4 * kq);
        t2_st4(img + rr * LD + 4 * kq, v);
    }
}

template <int TD>
__device__ __forceinline__ void sa_zero(f32x16 (&acc)[TD]) {
#pragma unroll
    for (int i = 0; i < TD; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// the lane's half of row `row` of a (.., D) output from a transposed accumulator: register r of tile td is column
// 32 td + 8 (r >> 2) + 4 lhi + (r & 3); `mul` scales, `live` false stores +0
template <int TD>
__device__ __forceinline__ void sa_store_row(float* row, const f32x16 (&acc)[TD], int lhi, float mul, bool live) {
#pragma unroll
    for (int td = 0; td < TD; ++td)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) v = make_float4(mul * acc[td][4 * g], mul * acc[td][4 * g + 1], mul * acc[td][4 * g + 2], mul * acc[td][4 * g + 3]);
            t2_st4(row + 32 * td + 8 * g + 4 * lhi, v);
        }
}

template <int D>
__global__ __launch_bounds__(256) void self_attn_fwd_kernel(SaArgs a) {
    constexpr int TD = D / 32, BN = SA_FWD_BN, LDK = BN + 1, LDV = D + 4;
    __shared__ __attribute__((aligned(16))) float Kk[D * LDK];
    __shared__ __attribute__((aligned(16))) float Vr[BN * LDV];
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int T = a.len ? t2_clamp_count(a.len[b], a.T) : a.T;
    const int row0 = blockIdx.x * SA_BM, t = row0 + wave * 32 + l31;
    float* orow = a.out + (((long long)b * a.T + t) * a.H + h) * D;
    float* lse = a.out_lse ? a.out_lse + ((long long)b * a.H + h) * a.T : nullptr;
    f32x16 acc[TD];
    sa_zero(acc);
    if (row0 >= T) {                                                        // uniform: a tile wholly in the padding
        if (t < a.T) {
            sa_store_row(orow, acc, lhi, 0.f, false);
            if (lse && !lhi) lse[t] = 0.f;
        }
        return;
    }
    float qf[D / 2];
    sa_frag<D>(a.q.p + b * a.q.sb + t * a.q.st + h * a.q.sh, t < T, lhi, qf);
    const float* kb = a.k.p + b * a.k.sb + h * a.k.sh;
    const float* vb = a.v.p + b * a.v.sb + h * a.v.sh;
    const float ninf = sa_ninf();
    float m = ninf, l = 0.f;
    for (int j0 = 0; j0 < T; j0 += BN) {
        __syncthreads();
        sa_stage_kmajor<D, BN>(Kk, kb, a.k.st, j0, T);
        sa_stage_rows<D, BN>(Vr, vb, a.v.st, j0, T);
        __syncthreads();
        f32x16 s[2];
        sa_zero(s);
#pragma unroll
        for (int kk = 0; kk < D / 2; ++kk)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
                s[tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kk[(2 * kk + lhi) * LDK + 32 * tm + l31], qf[kk], s[tm], 0, 0, 0);
        float mx = ninf;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float sv = j0 + 32 * tm + 2 * r + lhi < T ? __fmul_rn(a.scale, s[tm][r]) : ninf;
                s[tm][r] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));                                 // key j0 exists, so mx is finite
        const float m_new = fmaxf(m, mx), alpha = expf(m - m_new);
        float ps = 0.f;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = expf(s[tm][r] - m_new);                     // exactly 0 for a key at or beyond T
                s[tm][r] = p;
                ps = __fadd_rn(ps, p);
            }
        l = fmaf(l, alpha, ps);
        m = m_new;
#pragma unroll
        for (int td = 0; td < TD; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[td][r] = __fmul_rn(acc[td][r], alpha);
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int td = 0; td < TD; ++td)
                    acc[td] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vr[(32 * tm + 2 * r + lhi) * LDV + 32 * td + l31], s[tm][r], acc[td], 0, 0, 0);
    }
    const float lt = l + __shfl_xor(l, 32);
    if (t < a.T) {
        const bool live = t < T;
#pragma unroll
        for (int td = 0; td < TD; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[td][r] = acc[td][r] / lt;
        sa_store_row(orow, acc, lhi, 1.0f, live);
        if (lse && !lhi) lse[t] = live ? m + logf(lt) : 0.f;
    }
}

// dK and dV of the 128 keys of a workgroup; the queries pass in steps of 32
template <int D>
__global__ __launch_bounds__(256) void self_attn_bwd_kv_kernel(SaArgs a) {
    constexpr int TD = D / 32, BQ = SA_BWD_BN, LD = BQ + 1;
    __shared__ __attribute__((aligned(16))) float Qk[D * LD];
    __shared__ __attribute__((aligned(16))) float Gk[D * LD];
    __shared__ float ls[BQ], dl[BQ];
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int T = a.len ? t2_clamp_count(a.len[b], a.T) : a.T;
    const int row0 = blockIdx.x * SA_BM, j = row0 + wave * 32 + l31;
    const long long orow = (((long long)b * a.T + j) * a.H + h) * D;
    f32x16 dk[TD], dv[TD];
    sa_zero(dk);
    sa_zero(dv);
    if (row0 >= T) {                                                        // uniform
        if (j < a.T) {
            sa_store_row(a.dk + orow, dk, lhi, 0.f, false);
            sa_store_row(a.dv + orow, dv, lhi, 0.f, false);
        }
        return;
    }
    float kf[D / 2], vf[D / 2];
    sa_frag<D>(a.k.p + b * a.k.sb + j * a.k.st + h * a.k.sh, j < T, lhi, kf);
    sa_frag<D>(a.v.p + b * a.v.sb + j * a.v.st + h * a.v.sh, j < T, lhi, vf);
    const float* qb = a.q.p + b * a.q.sb + h * a.q.sh;
    const float* gb = a.g.p + b * a.g.sb + h * a.g.sh;
    const float* lse = a.lse + ((long long)b * a.H + h) * a.T;
    const float* delta = a.delta + ((long long)b * a.H + h) * a.T;
    for (int t0 = 0; t0 < T; t0 += BQ) {
        __syncthreads();
        sa_stage_kmajor<D, BQ>(Qk, qb, a.q.st, t0, T);
        sa_stage_kmajor<D, BQ>(Gk, gb, a.g.st, t0, T);
        if (threadIdx.x < BQ) {
            const int t = t0 + threadIdx.x;
            ls[threadIdx.x] = t < T ? lse[t] : 0.f;
            dl[threadIdx.x] = t < T ? delta[t] : 0.f;
        }
        __syncthreads();
        f32x16 s[1], dp[1];
        sa_zero(s);
        sa_zero(dp);
#pragma unroll
        for (int kk = 0; kk < D / 2; ++kk) {
            s[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qk[(2 * kk + lhi) * LD + l31], kf[kk], s[0], 0, 0, 0);
            dp[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gk[(2 * kk + lhi) * LD + l31], vf[kk], dp[0], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tt = 2 * r + lhi;
            const float p = (t0 + tt < T && j < T) ? expf(__fmul_rn(a.scale, s[0][r]) - ls[tt]) : 0.f;
            s[0][r] = p;
            dp[0][r] = __fmul_rn(p, dp[0][r] - dl[tt]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int slot = (r & 3) + 8 * (r >> 2) + 4 * lhi;              // sa_slot(2 r + lhi)
#pragma unroll
            for (int td = 0; td < TD; ++td) {
                dv[td] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gk[(32 * td + l31) * LD + slot], s[0][r], dv[td], 0, 0, 0);
                dk[td] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qk[(32 * td + l31) * LD + slot], dp[0][r], dk[td], 0, 0, 0);
            }
        }
    }
    if (j < a.T) {
        sa_store_row(a.dk + orow, dk, lhi, a.scale, j < T);
        sa_store_row(a.dv + orow, dv, lhi, 1.0f, j < T);
    }
}

// dQ of the 128 queries of a workgroup; the keys pass in steps of 32
template <int D>
__global__ __launch_bounds__(256) void self_attn_bwd_q_kernel(SaArgs a) {
    constexpr int TD = D / 32, BN = SA_BWD_BN, LD = BN + 1;
    __shared__ __attribute__((aligned(16))) float Kk[D * LD];
    __shared__ __attribute__((aligned(16))) float Vk[D * LD];
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int T = a.len ? t2_clamp_count(a.len[b], a.T) : a.T;
    const int row0 = blockIdx.x * SA_BM, t = row0 + wave * 32 + l31;
    float* orow = a.dq + (((long long)b * a.T + t) * a.H + h) * D;
    f32x16 dq[TD];
    sa_zero(dq);
    if (row0 >= T) {                                                        // uniform
        if (t < a.T) sa_store_row(orow, dq, lhi, 0.f, false);
        return;
    }
    float qf[D / 2], gf[D / 2];
    sa_frag<D>(a.q.p + b * a.q.sb + t * a.q.st + h * a.q.sh, t < T, lhi, qf);
    sa_frag<D>(a.g.p + b * a.g.sb + t * a.g.st + h * a.g.sh, t < T, lhi, gf);
    const float* kb = a.k.p + b * a.k.sb + h * a.k.sh;
    const float* vb = a.v.p + b * a.v.sb + h * a.v.sh;
    float lse_t = 0.f, dl_t = 0.f;
    if (t < T) {
        lse_t = a.lse[((long long)b * a.H + h) * a.T + t];
        dl_t = a.delta[((long long)b * a.H + h) * a.T + t];
    }
    for (int j0 = 0; j0 < T; j0 += BN) {
        __syncthreads();
        sa_stage_kmajor<D, BN>(Kk, kb, a.k.st, j0, T);
        sa_stage_kmajor<D, BN>(Vk, vb, a.v.st, j0, T);
        __syncthreads();
        f32x16 s[1], dp[1];
        sa_zero(s);
        sa_zero(dp);
#pragma unroll
        for (int kk = 0; kk < D / 2; ++kk) {
            s[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kk[(2 * kk + lhi) * LD + l31], qf[kk], s[0], 0, 0, 0);
            dp[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vk[(2 * kk + lhi) * LD + l31], gf[kk], dp[0], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = (j0 + 2 * r + lhi < T && t < T) ? expf(__fmul_rn(a.scale, s[0][r]) - lse_t) : 0.f;
            dp[0][r] = __fmul_rn(p, dp[0][r] - dl_t);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int slot = (r & 3) + 8 * (r >> 2) + 4 * lhi;
#pragma unroll
            for (int td = 0; td < TD; ++td)
                dq[td] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kk[(32 * td + l31) * LD + slot], dp[0][r], dq[td], 0, 0, 0);
        }
    }
    if (t < a.T) sa_store_row(orow, dq, lhi, a.scale, t < T);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
#define SA_LAUNCH(kern, D, grid, s, args)                                                                                  \
    do {                                                                                                                   \
        if ((D) == 32)                                                                                                     \
            T2_LAUNCH(kern<32>, grid, dim3(256), 0, s, args);                                                              \
        else if ((D) == 64)                                                                                                \
            T2_LAUNCH(kern<64>, grid, dim3(256), 0, s, args);                                                              \
        else if ((D) == 96)                                                                                                \
            T2_LAUNCH(kern<96>, grid, dim3(256), 0, s, args);                                                              \
        else                                                                                                               \
            T2_LAUNCH(kern<128>, grid, dim3(256), 0, s, args);                                                             \
    } while (0)

static int sa_inputs(const char* who, const SaOperand& q, const SaOperand& k, const SaOperand& v, int B, int T, int H, int D,
                     float scale) {
    char msg[160];
    T2_PROPAGATE(sa_check(who, B, T, H, D));
    T2_PROPAGATE(sa_check_operand(who, "q", q));
    T2_PROPAGATE(sa_check_operand(who, "k", k));
    T2_PROPAGATE(sa_check_operand(who, "v", v));
    if (!(scale > 0.0f && scale <= 3.0e38f)) {
        snprintf(msg, sizeof(msg), "self_attn: %s: the scale must be positive and finite", who);
        T2_FAIL(msg);
    }
    return T2AMD_OK;
}

// does the contiguous output [out, out + bytes) share a byte with one of the three inputs
static bool sa_hits_inputs(const void* out, long long bytes, const SaOperand& q, const SaOperand& k, const SaOperand& v, int B, int T,
                           int H, int D) {
    return t2_overlap(out, bytes, q.p, sa_span(q, B, T, H, D)) || t2_overlap(out, bytes, k.p, sa_span(k, B, T, H, D)) ||
           t2_overlap(out, bytes, v.p, sa_span(v, B, T, H, D));
}

extern "C" int t2amd_self_attn_f32(const float* q, long long qb, long long qt, long long qh, const float* k, long long kb, long long kt,
                                   long long kh, const float* v, long long vb, long long vt, long long vh, const int* lengths, int B,
                                   int T, int H, int D, float scale, float* o, float* lse, void* stream) {
    const SaOperand qo = {q, qb, qt, qh}, ko = {k, kb, kt, kh}, vo = {v, vb, vt, vh};
    T2_PROPAGATE(sa_inputs("forward", qo, ko, vo, B, T, H, D, scale));
    T2_REQUIRE(o, "self_attn: forward: null operand");
    T2_REQUIRE(t2_aligned16(o), "self_attn: forward: o is not aligned to 16 bytes");
    const long long obytes = 4LL * B * T * H * D, lbytes = 4LL * B * H * T;
    T2_REQUIRE(!sa_hits_inputs(o, obytes, qo, ko, vo, B, T, H, D) && !(lse && sa_hits_inputs(lse, lbytes, qo, ko, vo, B, T, H, D)) &&
                   !(lse && t2_overlap(lse, lbytes, o, obytes)),
               "self_attn: forward: the outputs must not overlap the inputs or each other");
    SaArgs a = {};
    a.q = qo; a.k = ko; a.v = vo; a.out = o; a.out_lse = lse; a.len = lengths; a.T = T; a.H = H; a.scale = scale;
    const dim3 grid((unsigned)t2_cdiv(T, SA_BM), (unsigned)(B * H));
    SA_LAUNCH(self_attn_fwd_kernel, D, grid, (hipStream_t)stream, a);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_self_attn_bwd_f32(const float* q, long long qb, long long qt, long long qh, const float* k, long long kb,
                                       long long kt, long long kh, const float* v, long long vb, long long vt, long long vh,
                                       const float* o, const float* lse, const float* g, long long gb, long long gt, long long gh,
                                       const int* lengths, int B, int T, int H, int D, float scale, float* dq, float* dk, float* dv,
                                       unsigned char* ws, long long ws_bytes, void* stream) {
    const SaOperand qo = {q, qb, qt, qh}, ko = {k, kb, kt, kh}, vo = {v, vb, vt, vh}, go = {g, gb, gt, gh};
    T2_PROPAGATE(sa_inputs("backward", qo, ko, vo, B, T, H, D, scale));
    T2_PROPAGATE(sa_check_operand("backward", "the gradient", go));
    T2_REQUIRE(o && lse && dq && dk && dv && ws, "self_attn: backward: null operand");
    T2_REQUIRE(ws_bytes >= sa_rows_bytes(B, T, H), "self_attn: backward: the workspace is smaller than t2amd_self_attn_workspace asks for");
    T2_REQUIRE(t2_aligned16(ws) && t2_aligned16(dq) && t2_aligned16(dk) && t2_aligned16(dv) && t2_aligned16(o),
               "self_attn: backward: o, dq, dk, dv and the workspace must be aligned to 16 bytes");
    const long long obytes = 4LL * B * T * H * D, lbytes = 4LL * B * H * T, gspan = sa_span(go, B, T, H, D);
    float* outs[4] = {dq, dk, dv, reinterpret_cast<float*>(ws)};
    const long long obs[4] = {obytes, obytes, obytes, ws_bytes};
    bool clash = false;
    for (int i = 0; i < 4; ++i) {
        clash = clash || sa_hits_inputs(outs[i], obs[i], qo, ko, vo, B, T, H, D) || t2_overlap(outs[i], obs[i], g, gspan) ||
                t2_overlap(outs[i], obs[i], o, obytes) || t2_overlap(outs[i], obs[i], lse, lbytes);
        for (int j2 = i + 1; j2 < 4; ++j2) clash = clash || t2_overlap(outs[i], obs[i], outs[j2], obs[j2]);
    }
    T2_REQUIRE(!clash, "self_attn: backward: outputs and workspace must not overlap the inputs or each other");
    float* delta = reinterpret_cast<float*>(ws);
    T2_PROPAGATE(t2amd_self_attn_delta_f32(g, gb, gt, gh, o, lengths, B, T, H, D, delta, stream));
    SaArgs a = {};
    a.q = qo; a.k = ko; a.v = vo; a.g = go; a.o = o; a.lse = lse; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv;
    a.len = lengths; a.T = T; a.H = H; a.scale = scale;
    const dim3 grid((unsigned)t2_cdiv(T, SA_BM), (unsigned)(B * H));
    SA_LAUNCH(self_attn_bwd_kv_kernel, D, grid, (hipStream_t)stream, a);
    SA_LAUNCH(self_attn_bwd_q_kernel, D, grid, (hipStream_t)stream, a);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
