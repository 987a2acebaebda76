// Multi-resolution STFT loss (tacotron2_amd/audio.py MultiResolutionSTFTLoss).  Per resolution r the two
// spectra spec_x, spec_y (B n, 2F) rows [re | im] come from the forward GEMM of gemm.hip; this file holds the row passes of the
// loss on top of them and the sum of the R sample gradients, one launch each:
//   stft_loss_fwd:    p = re^2 + im^2, m = sqrt(max(p, eps)) for x and y; per workgroup one partial slot of three float64 sums
//                     over the frames j < cnt[b]:  sum (m_y - m_x)^2,  sum m_y^2,  sum |ln m_x - ln m_y|.
//   stft_loss_finish: one launch after all resolutions: adds every resolution's slots in a fixed order in float64 and writes
//                     the loss, the (R, 2) terms (sc_r, lm_r) and the (R, 2) coefficients of the backward
//                     (sc_weight / (R sqrt(A) sqrt(Bn)), 0 where A == 0, and mag_weight / (R C)).  No host read in between.
//   stft_loss_bwd:    d_m = c_sc (m_x - m_y) + c_mag sign(ln m_x - ln m_y) / m_x, d_re = g d_m re / m_x, d_im = g d_m im / m_x
//                     where p >= eps (torch's clamp rule: the gradient passes at equality), exactly 0 below and on the frames
//                     outside the mask; m recomputed by the forward's operations in the forward's order (t2_power, sl_mag).
//                     The rows of d_spec are t2_dspec_store's (common.h), as magnitude_bwd_kernel's.
//   stft_loss_sum:    d_y = ((part_0 + part_1) + ...) + part_{R-1}, one writer per sample.
// No atomics anywhere: every output element has one writer and every sum a fixed order, so two calls give the same bits.
// No MFMA and no LDS-DMA here, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
//
// Access widths.  A spec row has 2F = L + 2 floats: its start is 16-byte aligned every other row only and its imaginary half
// starts at an odd float, so the kernels take one bin per lane with 4-byte accesses, every wave
// instruction one contiguous 256-byte run on each of its streams.
#include "common.h"

#define SL_MAX_RES 8                    /* resolutions of one stft_loss_finish / stft_loss_sum launch */
#define SL_SLOT_ELEMS 16384             /* about this many bins per partial slot */

__device__ __forceinline__ float sl_mag(float p, float eps) { return sqrtf(fmaxf(p, eps)); }

// ---- forward sums ------------------------------------------------------------------------------------------------------
// A workgroup owns `rpb` consecutive frame rows: a thread adds its bins (f = tid, tid + 256, ...) row after row in float64, the
// wave butterfly and the four wave sums follow in a fixed order, and thread 0 stores the three sums as the workgroup's slot.
__global__ void __launch_bounds__(256) stft_loss_fwd_kernel(const float* __restrict__ spec_x, long long ldx,
                                                            const float* __restrict__ spec_y, long long ldy,
                                                            const int* __restrict__ cnt, int n, int F, long long rows, int rpb,
                                                            float eps, double* __restrict__ slots) {
    __shared__ double wsum[3][4];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * rpb;
    double a = 0.0, bn = 0.0, lm = 0.0;
    for (int rr = 0; rr < rpb; ++rr) {
        const long long row = row0 + rr;
        if (row >= rows) break;
        const long long b = row / n;
        if ((int)(row - b * n) >= t2_clamp_count(cnt[(int)b], n)) continue;
        const float* px = spec_x + row * ldx;
        const float* py = spec_y + row * ldy;
        for (int f = tid; f < F; f += 256) {
            const float mx = sl_mag(t2_power(px[f], px[F + f]), eps);
            const float my = sl_mag(t2_power(py[f], py[F + f]), eps);
            const double d = (double)my - (double)mx;
            a += d * d;
            bn += (double)my * (double)my;
            lm += (double)fabsf(logf(mx) - logf(my));
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m);
        bn += __shfl_xor(bn, m);
        lm += __shfl_xor(lm, m);
    }
    if ((tid & 63) == 0) {
        wsum[0][tid >> 6] = a;
        wsum[1][tid >> 6] = bn;
        wsum[2][tid >> 6] = lm;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) slots[3 * (long long)blockIdx.x + k] = t2_block_total_f64(wsum[k]);
    }
}

extern "C" int t2amd_stft_loss_rows_per_slot(int F) {
    if (F < 1) F = 1;
    return F >= SL_SLOT_ELEMS ? 1 : (SL_SLOT_ELEMS + F - 1) / F;
}

extern "C" int t2amd_stft_loss_fwd_f32(const float* spec_x, long long ldx, const float* spec_y, long long ldy, const int* cnt,
                                       int B, int n, int F, float eps, double* slots, long long slot_doubles, void* stream) {
    T2_REQUIRE(spec_x && spec_y && cnt && slots, "stft_loss_fwd: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && n > 0 && F > 0 && F <= 65536, "stft_loss_fwd: bad dims");
    T2_REQUIRE((long long)B * n <= T2_MAX_ROWS, "stft_loss_fwd: at most 2^31 - 256 frame rows");
    T2_REQUIRE(ldx >= 2 * (long long)F && ldy >= 2 * (long long)F, "stft_loss_fwd: row too short");
    T2_REQUIRE(eps > 0.0f, "stft_loss_fwd: eps must be positive");
    const long long rows = (long long)B * n;
    const int rpb = t2amd_stft_loss_rows_per_slot(F);
    const long long nslots = (rows + rpb - 1) / rpb;
    T2_REQUIRE(slot_doubles >= 3 * nslots, "stft_loss_fwd: the slot buffer is shorter than its 3 doubles per slot");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(slots) & 7u) == 0, "stft_loss_fwd: the slot buffer is misaligned");
    T2_REQUIRE(!t2_overlap(slots, 3 * nslots * 8, spec_x, ((rows - 1) * ldx + 2 * (long long)F) * 4) &&
                   !t2_overlap(slots, 3 * nslots * 8, spec_y, ((rows - 1) * ldy + 2 * (long long)F) * 4),
               "stft_loss_fwd: the slot buffer must not be one of the inputs");
    T2_LAUNCH(stft_loss_fwd_kernel, dim3((unsigned)nslots), dim3(256), 0, (hipStream_t)stream, spec_x, ldx, spec_y, ldy, cnt, n, F,
              rows, rpb, eps, slots);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- finish ------------------------------------------------------------------------------------------------------------
// One workgroup.  Resolution r owns the slots [off[r], off[r + 1]): thread t adds slots t, t + 256, ... in ascending order, the
// butterfly and the four wave sums follow, thread 0 combines.  count[r] = C_r = F_r sum_b n_{r,b}.
struct sl_finish_plan {
    long long off[SL_MAX_RES + 1];
    double count[SL_MAX_RES];
};

__global__ void __launch_bounds__(256) stft_loss_finish_kernel(const double* __restrict__ slots, sl_finish_plan plan, int R,
                                                               float sc_weight, float mag_weight, float* __restrict__ loss,
                                                               float* __restrict__ terms, float* __restrict__ coef) {
    __shared__ double wsum[3][4];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int r = 0; r < R; ++r) {
        double s[3] = {0.0, 0.0, 0.0};
        for (long long i = plan.off[r] + tid; i < plan.off[r + 1]; i += 256) {
            s[0] += slots[3 * i + 0];
            s[1] += slots[3 * i + 1];
            s[2] += slots[3 * i + 2];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            s[0] += __shfl_xor(s[0], m);
            s[1] += __shfl_xor(s[1], m);
            s[2] += __shfl_xor(s[2], m);
        }
        if ((tid & 63) == 0) {
            wsum[0][tid >> 6] = s[0];
            wsum[1][tid >> 6] = s[1];
            wsum[2][tid >> 6] = s[2];
        }
        __syncthreads();
        if (tid == 0) {
            const double A = t2_block_total_f64(wsum[0]), Bn = t2_block_total_f64(wsum[1]), Lm = t2_block_total_f64(wsum[2]);
            const double ra = sqrt(A), rb = sqrt(Bn);
            const double sc = A == 0.0 ? 0.0 : ra / rb;                 // a definition: no gradient and no value where A == 0
            const double lmr = Lm / plan.count[r];
            terms[2 * r + 0] = (float)sc;
            terms[2 * r + 1] = (float)lmr;
            coef[2 * r + 0] = A == 0.0 ? 0.0f : (float)((double)sc_weight / ((double)R * ra * rb));
            coef[2 * r + 1] = (float)((double)mag_weight / ((double)R * plan.count[r]));
            total += (double)sc_weight * sc + (double)mag_weight * lmr;
        }
        __syncthreads();                                                // wsum is written again by the next resolution
    }
    if (tid == 0) loss[0] = (float)(total / (double)R);
}

extern "C" int t2amd_stft_loss_finish_f64(const double* slots, long long slot_doubles, const long long* slot_off,
                                          const double* counts, int R, float sc_weight, float mag_weight, float* loss,
                                          float* terms, float* coef, void* stream) {
    T2_REQUIRE(slots && slot_off && counts && loss && terms && coef, "stft_loss_finish: null operand");
    T2_REQUIRE(R >= 1 && R <= SL_MAX_RES, "stft_loss_finish: 1 to 8 resolutions");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(slots) & 7u) == 0, "stft_loss_finish: the slot buffer is misaligned");
    sl_finish_plan plan;
    for (int r = 0; r <= SL_MAX_RES; ++r) plan.off[r] = 0;
    for (int r = 0; r < SL_MAX_RES; ++r) plan.count[r] = 1.0;
    T2_REQUIRE(slot_off[0] >= 0, "stft_loss_finish: slot offsets must ascend from a non-negative start");
    for (int r = 0; r < R; ++r) {
        T2_REQUIRE(slot_off[r + 1] > slot_off[r], "stft_loss_finish: slot offsets must ascend, at least one slot per resolution");
        T2_REQUIRE(counts[r] > 0.0, "stft_loss_finish: a resolution's count must be positive");
        plan.count[r] = counts[r];
    }
    for (int r = 0; r <= R; ++r) plan.off[r] = slot_off[r];
    T2_REQUIRE(slot_off[R] <= slot_doubles / 3, "stft_loss_finish: the slot buffer is shorter than its 3 doubles per slot");
    T2_REQUIRE(loss != terms && loss != coef && terms != coef, "stft_loss_finish: the outputs must be distinct");
    T2_REQUIRE(!t2_overlap(slots, slot_doubles * 8, loss, 4) && !t2_overlap(slots, slot_doubles * 8, terms, 8LL * R) &&
                   !t2_overlap(slots, slot_doubles * 8, coef, 8LL * R),
               "stft_loss_finish: an output must not lie in the slot buffer");
    T2_LAUNCH(stft_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, slots, plan, R, sc_weight, mag_weight, loss, terms,
              coef);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// Lane = bin f of row r, as magnitude_bwd_kernel; the row of d_spec is t2_dspec_store's (common.h).  coef = this resolution's
// (c_sc, c_mag), g = the upstream scalar, both read on the device.
__global__ void __launch_bounds__(256) stft_loss_bwd_kernel(const float* __restrict__ spec_x, long long ldx,
                                                            const float* __restrict__ spec_y, long long ldy,
                                                            const int* __restrict__ cnt, const float* __restrict__ coef,
                                                            const float* __restrict__ g, int n, long long rows, int F, int Kp,
                                                            float eps, float* __restrict__ d_spec, long long ldd) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * F) return;
    const long long r = i / F;
    const int f = (int)(i - r * F);
    const long long b = r / n;
    float dre = 0.0f, dim = 0.0f;
    if ((int)(r - b * n) < t2_clamp_count(cnt[(int)b], n)) {
        const float re = spec_x[r * ldx + f], im = spec_x[r * ldx + F + f];
        const float p = t2_power(re, im);
        if (p >= eps) {
            const float mx = sl_mag(p, eps);
            const float my = sl_mag(t2_power(spec_y[r * ldy + f], spec_y[r * ldy + F + f]), eps);
            const float d = logf(mx) - logf(my);
            const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            const float up = g[0];
            const float dm = __fadd_rn(__fmul_rn(__fmul_rn(up, coef[0]), mx - my), __fmul_rn(__fmul_rn(up, coef[1]), sg) / mx);
            const float q = dm / mx;
            dre = __fmul_rn(q, re);
            dim = __fmul_rn(q, im);
        }
    }
    t2_dspec_store(d_spec, r * ldd, f, F, Kp, dre, dim);
}

extern "C" int t2amd_stft_loss_bwd_f32(const float* spec_x, long long ldx, const float* spec_y, long long ldy, const int* cnt,
                                       const float* coef, const float* g, int B, int n, int F, int Kp, float eps, float* d_spec,
                                       long long ldd, long long d_floats, void* stream) {
    T2_REQUIRE(spec_x && spec_y && cnt && coef && g && d_spec, "stft_loss_bwd: null operand");
    T2_REQUIRE(B > 0 && B <= 65535 && n > 0 && F > 0 && F <= 65536, "stft_loss_bwd: bad dims");
    T2_REQUIRE((long long)B * n <= T2_MAX_ROWS, "stft_loss_bwd: at most 2^31 - 256 frame rows");
    T2_REQUIRE(ldx >= 2 * (long long)F && ldy >= 2 * (long long)F, "stft_loss_bwd: row too short");
    T2_REQUIRE(eps > 0.0f, "stft_loss_bwd: eps must be positive");
    const long long rows = (long long)B * n;
    unsigned blocks;
    T2_PROPAGATE(t2_dspec_blocks("stft_loss_bwd", rows, F, Kp, ldd, &blocks));
    T2_REQUIRE(d_floats >= (rows - 1) * ldd + Kp, "stft_loss_bwd: d_spec is shorter than its B n rows of Kp");
    const long long d_bytes = ((rows - 1) * ldd + Kp) * 4;
    T2_REQUIRE(!t2_overlap(d_spec, d_bytes, spec_x, ((rows - 1) * ldx + 2 * (long long)F) * 4) &&
                   !t2_overlap(d_spec, d_bytes, spec_y, ((rows - 1) * ldy + 2 * (long long)F) * 4) &&
                   !t2_overlap(d_spec, d_bytes, coef, 8) && !t2_overlap(d_spec, d_bytes, g, 4),
               "stft_loss_bwd: d_spec must not be one of the inputs");
    T2_LAUNCH(stft_loss_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, spec_x, ldx, spec_y, ldy, cnt, coef, g, n, rows,
              F, Kp, eps, d_spec, ldd);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

// ---- the R sample gradients, summed in the order r = 0 .. R - 1 ----------------------------------------------------------------
__global__ void __launch_bounds__(256) stft_loss_sum_kernel(const float* __restrict__ parts, long long stride, int R,
                                                            long long total, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float acc = parts[i];
    for (int r = 1; r < R; ++r) acc = __fadd_rn(acc, parts[r * stride + i]);
    out[i] = acc;
}

extern "C" int t2amd_stft_loss_sum_f32(const float* parts, long long stride, long long part_floats, int R, long long total,
                                       float* out, void* stream) {
    T2_REQUIRE(parts && out, "stft_loss_sum: null operand");
    T2_REQUIRE(R >= 1 && R <= SL_MAX_RES, "stft_loss_sum: 1 to 8 parts");
    T2_REQUIRE(total > 0 && stride >= total, "stft_loss_sum: bad dims");
    T2_REQUIRE(part_floats >= (R - 1) * stride + total, "stft_loss_sum: parts is shorter than its R images");
    T2_REQUIRE(!t2_overlap(out, total * 4, parts, ((R - 1) * stride + total) * 4), "stft_loss_sum: out must not lie in parts");
    const long long blocks = (total + 255) / 256;
    T2_REQUIRE(blocks <= 0x7fffffffLL, "stft_loss_sum: too many elements for one launch");
    T2_LAUNCH(stft_loss_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, parts, stride, R, total, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
