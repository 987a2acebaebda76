/*
 * tacotron2_amd.h — C ABI of the MI355X (gfx950) Tacotron 2 mel-spectrogram engine.
 *
 * The reference (NVIDIA/tacotron2) has no FFI/plugin interface: its hot path is Python
 * (`model.py`) over PyTorch/cuDNN/NCCL.  This header is the boundary the
 * reference *would* bind if its `model.py` delegated to a native library: every entry
 * point below names the reference lines whose arithmetic it replaces.  The Python host
 * (`tacotron2_amd/model.py`, same class/method/state_dict surface as reference
 * model.py:457-529) binds these symbols with ctypes; a maintainer of the reference would
 * add exactly the same ctypes stubs.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types.  All tensors are fp32 row-major
 *     in HBM unless stated; `ld*` are row strides in ELEMENTS; masks are uint8 keep-masks
 *     (1 = keep) applied as x * keep * keep_scale (keep_scale = 1/(1-p) formed in fp32).
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream) and returns immediately: T2AMD_OK or an error code; the message is
 *     available from t2amd_last_error().  Nothing allocates or frees device memory: the
 *     caller owns all buffers, including workspaces (graph-capture safe).
 *   - time-major slabs: [T][B][F]; batch-major: [B][T][F].
 */
#ifndef TACOTRON2_AMD_H
#define TACOTRON2_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2AMD_ABI_VERSION 1
#define T2AMD_OK 0
#define T2AMD_ERR_ARG 1
#define T2AMD_ERR_LAUNCH 2

/* attention geometry compiled into the kernels (reference hparams.py:66-70 defaults) */
#define T2AMD_ATT_DIM 128
#define T2AMD_LOC_FILTERS 32
#define T2AMD_LOC_KERNEL 31
#define T2AMD_LOC_TAPS (2 * T2AMD_LOC_KERNEL) /* 62 = [prev ; cumulative] x 31 */
#define T2AMD_ATT_SLICES 4 /* workgroups per utterance in every attention kernel; partial slabs have this many slices */

int t2amd_abi_version(void);
/* SHA-1 (40 hex digits) over csrc/ and this header, compiled in by tacotron2_amd/build.py: the binding refuses a library
 * that was not built from the sources beside it, and bench.py prints it next to the hash recorded with the PMC passes. */
const char* t2amd_source_sha1(void);
const char* t2amd_last_error(void);
/* sizeof() of every struct below, in declaration order, for binding self-checks. */
int t2amd_struct_sizes(int* out, int max_n);
/* Validate-only mode: all argument checks and host loops run, no kernel is launched (outputs are
 * left untouched).  For CPU-side tests of the binding; not a compute path. */
int t2amd_set_validate_only(int on);
/* Live kernel timing for bench.py's roofline: while enabled, every LSTM-step launch whose tag equals
 * `tag` is bracketed by two hipEvents on its own stream (at most `max_launches` launches).
 * t2amd_profile_read synchronises those events and returns the summed elapsed time and the count. */
int t2amd_profile_enable(int tag, int max_launches);
int t2amd_profile_read(float* total_ms, int* count);
/* Elapsed time of an EMPTY bracket (two event records back to back on the launch stream), measured at the start
 * of the profiling session: what a bracket costs besides the kernel.  Call before t2amd_profile_read. */
int t2amd_profile_event_overhead(float* ms);

/* ------------------------------------------------------------------------------------
 * Dense / implicit-convolution GEMM on exact-f32 MFMA (v_mfma_f32_32x32x2_f32).
 *   C[M,N] (+)= act(A[M,K] . B[K,N] + bias[N]) * keep * keep_scale
 * replaces every torch.nn.Linear / Conv1d forward, dgrad and wgrad on the path:
 * reference layers.py:17-18,37-39 (LinearNorm/ConvNorm.forward), model.py:99 (Prenet),
 * :141-146 (Postnet convs), :174-175 (Encoder convs), :288 (memory_layer), :375-378
 * (linear_projection + gate_layer) and autograd's matching backward GEMMs.
 * ------------------------------------------------------------------------------------ */
typedef struct t2amd_gemm_desc {
    const float* A;
    const float* B;
    float* C;
    int M, N, K;
    long long lda, ldb, ldc;
    int a_kcontig;   /* 1: A stored [M][K] (K contiguous); 0: A stored [K][M] */
    int b_kcontig;   /* 1: B stored [N][K] (K contiguous, the nn.Linear weight layout); 0: [K][N] */
    int batch;       /* >=1 independent problems, pointers advance by stride* */
    long long strideA, strideB, strideC;
    int splitk;      /* >=1; when >1 the kernel writes `splitk` partial C's (stride strideSplitC)
                        with a plain store and the epilogue fields must be unset */
    long long strideSplitC;
    int accumulate;  /* 1: C += result */
    const float* bias;      /* [N] or NULL */
    int act;                /* 0 none, 1 relu */
    const uint8_t* keep;    /* [M][ldkeep] or NULL */
    long long ldkeep;
    float keep_scale;
    /* implicit 1-D convolution over channel-last rows r = b*T + t (stride 1, 'same' zero pad):
     * A-side (needs a_kcontig=1): K = taps*convA_C, column (tap,c) of row r reads
     *   A[(r + (tap-pad)*sign)*lda + c] if 0 <= t + (tap-pad)*sign < T else 0.
     * B-side (needs b_kcontig=0, used by wgrad): N = taps*convB_C, column (tap,c) of K-row r reads
     *   B[(r + tap - pad)*ldb + c] if 0 <= t + tap - pad < T else 0. */
    int convA_T, convA_C, convA_pad, convA_sign;
    int convB_T, convB_C, convB_pad;
    /* 0: exact f32 MFMA (bitwise an fmaf chain).  1: split-bf16: A = Ah+Al, B = Bh+Bl in bf16, product =
     * Ah.Bh + Ah.Bl + Al.Bh on the bf16 MFMA with f32 accumulation (~2^-17 relative per product, 5.3x the
     * f32 MFMA ceiling).  The engine requests 1 for gradient GEMMs in f32 mode.  2: plain bf16 product
     * (operands rounded to bf16, f32 accumulation) — the engine's bf16 compute mode. */
    int precision;
} t2amd_gemm_desc;

/* Output tile edge (128 or 256) t2amd_gemm_f32 will use for an M x N product at `precision` with the given
 * operand layouts, launched as `nz` = batch*splitk slices: callers that split K pick the split count from the resulting workgroup count.
 * (Host-side sizing helper; the reference has no counterpart, torch.mm hides its tiling.) */
int t2amd_gemm_tile_size(int M, int N, int precision, int nz, int a_kcontig, int b_kcontig);
int t2amd_gemm_f32(const t2amd_gemm_desc* d, void* stream);

/* out[i] (+)= sum_s partials[s*stride + i]; with `perm_taps`>0 the flat index i = (co, tap, ci)
 * is written to (co, ci, tap) (packed conv-weight grad -> torch Conv1d layout, Ci = perm_ci). */
int t2amd_splitk_reduce_f32(const float* partials, int nsplit, long long stride, float* out,
                            long long n, int accumulate, int perm_taps, int perm_ci, void* stream);
/* out[r][c] (row stride ldo >= cols) (+)= sum_s partials[s*stride + r*cols + c]: partials of a product that fills a column
 * block of a wider matrix. */
int t2amd_splitk_reduce2d_f32(const float* partials, int nsplit, long long stride, float* out, int rows, int cols,
                              long long ldo, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * bf16-resident product (csrc/gemm16.hip): C[M][N] (f32) = A[M][K] . B[N][K]^T (+ bias[n]), A and B bf16 and
 * K-contiguous (row strides lda / ldb in elements, multiples of 8, >= K), K a multiple of 64.  In the bf16 compute mode
 * it carries the products whose operands exist as bf16 images: the deferred weight gradients dW = dG^T . X of the
 * decoder LSTMs and of the hoisted input projection (reference model.py:352-371 under autograd) on K-contiguous images
 * made by t2amd_transpose_cast_bf16.  splitk > 1 writes partial slabs strideSplitC apart (plain epilogue only).
 * ------------------------------------------------------------------------------------ */
typedef struct t2amd_gemm16_desc {
    const void* A;          /* [M][lda] bf16 */
    const void* B;          /* [N][ldb] bf16 */
    float* C;               /* [splitk][M][ldc] f32 */
    int M, N, K;
    long long lda, ldb, ldc;
    int splitk;
    long long strideSplitC;
    int accumulate;         /* C += (splitk must be 1) */
    const float* bias;      /* [N] or NULL (splitk must be 1) */
    /* window mode (win_Tp > 0; nn.Conv1d over channel-last rows, reference layers.py:37-39 / model.py:141-146, 174-175):
     * A is a bf16 image [B][Tp = T + 2 pad][Ci] with zero halo rows (t2amd_cast_halo_bf16), lda = Ci, K = k Ci rounded up to 64
     * (B's columns behind k Ci zero, t2amd_pack_conv_bf16; the windows' overhang stays inside the image's last halo) -- row
     * m = b Tp + t of A is the k-tap window of output (b, t), overlapping its neighbours; M = B Tp window rows are
     * multiplied and those with t < win_T are stored to the compact rows b win_T + t of C.  splitk must be 1. */
    int win_T, win_Tp;
} t2amd_gemm16_desc;
int t2amd_gemm16_tn(const t2amd_gemm16_desc* d, void* stream);
/* The same product with K-MAJOR operands: C[M][N] = sum_k A[k][m] . B[k][n], A = [K][lda], B = [K][ldb] bf16 with m / n
 * contiguous -- the layout of the time loops' [To.B][.] slabs and of channel-last activation images, so the weight gradients
 * dW = dG^T . X of nn.LSTMCell (reference model.py:352-371 under autograd) and nn.Conv1d (layers.py:37-39) need no
 * transposed copies; fragments are formed by gfx950's transposing LDS read.  M, N multiples of 8; lda / ldb multiples of 8
 * and possibly SMALLER than M / N (overlapping rows: B[k][n] = img[k Ci + n], n < taps Ci, is the sliding window of a
 * convolution over a channel-last image); any K > 0; win_T = win_Tp = 0; bias / accumulate / splitk as above. */
int t2amd_gemm16_kk(const t2amd_gemm16_desc* d, void* stream);
/* Up to four such products in ONE launch (same M, same splitk; each with its own A offset / K / B / C): their workgroups run
 * side by side on the same rows of A, which is then read once -- the input blocks [x | ctx | h] of an LSTM's weight gradient. */
int t2amd_gemm16_kk_group(const t2amd_gemm16_desc* d, int count, void* stream);

/* dst[(b (T + 2 pad) + pad + t)][c] (bf16) = src[(b T + t)][c]; dst ([B (T + 2 pad) + 2 pad][C]; every row is written, the halo
 * rows with zeros: it need not be initialised) is the image the window mode reads. */
int t2amd_cast_halo_bf16(const float* src, long long lds, void* dst, long long rows, int C, int T, int pad, void* stream);

/* bf16 weight image of nn.Conv1d (W f32 [Co][Ci][k], reference layers.py:37-39) for the window mode, Kp >= row length, the
 * columns behind it zero: reversed = 0 -> out[Co][Kp], out[co][tap Ci + ci] = W[co][ci][tap] (forward);
 * reversed = 1 -> out[Ci][Kp], out[ci][(k - 1 - tap) Co + co] = W[co][ci][tap] (data gradient: windows of g's image). */
int t2amd_pack_conv_bf16(const float* W, void* out, int Co, int Ci, int k, int Kp, int reversed, void* stream);

/* dst[c][r] (bf16, row stride ldd >= rows_padded; columns rows..rows_padded-1 zeroed) = src[r][c]; src is f32
 * (src_is_bf16 = 0) or bf16, row stride lds elements: the K-contiguous image of a [rows][cols] slab. */
int t2amd_transpose_cast_bf16(const void* src, int src_is_bf16, long long lds, void* dst, long long ldd, int rows, int cols,
                              int rows_padded, void* stream);

/* ------------------------------------------------------------------------------------
 * BatchNorm1d (+activation +dropout) over channel-last rows; replaces nn.BatchNorm1d +
 * relu/tanh + F.dropout in reference model.py:141-146, 174-175 (train: biased batch
 * variance for normalisation, unbiased for the running update, momentum 0.1, eps 1e-5).
 * ------------------------------------------------------------------------------------ */
/* column statistics of x[M][N] -> mean, invstd (=1/sqrt(var_biased+eps)); updates running
 * stats if non-NULL.  ws: >= 2*64*N doubles. */
int t2amd_bn_stats_f32(const float* x, long long ldx, int M, int N, double* ws, float* mean,
                       float* invstd, float* running_mean, float* running_var, float momentum,
                       float eps, void* stream);
/* invstd from running variance (eval mode): invstd = 1/sqrt(var+eps) */
int t2amd_bn_eval_invstd_f32(const float* running_var, float* invstd, int N, float eps, void* stream);
/* y = act((x-mean)*invstd*gamma+beta) * keep*scale ; act: 0 none, 1 relu, 2 tanh.
 * `row_valid_T`>0 with `lens`!=NULL zeroes rows whose t >= lens[b] (batched ragged inference). */
int t2amd_bn_act_fwd_f32(const float* x, long long ldx, float* y, long long ldy, int M, int N,
                         const float* mean, const float* invstd, const float* gamma,
                         const float* beta, int act, const uint8_t* keep, long long ldkeep,
                         float keep_scale, const int* lens, int row_valid_T, void* stream);
/* The same, with y leaving ALSO as the bf16 halo image the next convolution's window product reads (round 6; y_img16:
 * [M/T (T + 2 pad) + 2 pad][N], t2amd_cast_halo_bf16's layout, halo rows zeroed here; same bits as the cast pass over y).
 * Needs N % 4 == 0, 16-byte-aligned rows, M a multiple of T, T >= 2 pad. */
int t2amd_bn_act_fwd_img_f32(const float* x, long long ldx, float* y, long long ldy, int M, int N, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, int act, const uint8_t* keep,
                             long long ldkeep, float keep_scale, void* y_img16, int T, int pad, void* stream);
/* backward of the above (train mode).  dy is overwritten with dx (grad wrt the conv output x).
 * y = forward output (post activation/dropout).  dgamma/dbeta are written (not accumulated).
 * ws: >= 2*64*N doubles. */
int t2amd_bn_act_bwd_f32(float* dy, long long lddy, const float* y, long long ldy, const float* x,
                         long long ldx, int M, int N, const float* mean, const float* invstd,
                         const float* gamma, int act, const uint8_t* keep, long long ldkeep,
                         float keep_scale, double* ws, float* dgamma, float* dbeta, void* stream);
/* The same backward with its two followers folded into stage 2 (round 6; the bf16 mode's convolution backward, reference
 * layers.py:37-39 + model.py:141-146 under autograd): dx leaves as the bf16 halo image the window products read
 * (dx_img16: [M/T (T + 2 pad) + 2 pad][N], t2amd_cast_halo_bf16's layout, halo rows zeroed here) and as its column sums
 * (dbias[N]: the convolution's bias gradient, bit-identical to t2amd_colsum_f32 over dx) -- one pass instead of three over the
 * slab.  keep_f32 = 0: dy is left holding stage 1's intermediate (no f32 dx is written); 1: dy = dx as above.
 * Needs N % 4 == 0, 16-byte-aligned rows, M a multiple of T, T >= 2 pad. */
int t2amd_bn_act_bwd_img_f32(float* dy, long long lddy, const float* y, long long ldy, const float* x, long long ldx, int M, int N,
                             const float* mean, const float* invstd, const float* gamma, int act, const uint8_t* keep,
                             long long ldkeep, float keep_scale, double* ws, float* dgamma, float* dbeta, void* dx_img16, int T,
                             int pad, float* dbias, int keep_f32, void* stream);
/* column sums: out[N] (+)= sum_m x[m][n]  (bias gradients). ws >= 64*N doubles */
int t2amd_colsum_f32(const float* x, long long ldx, int M, int N, double* ws, float* out,
                     int accumulate, void* stream);
/* The same sums over a bf16 slab x16[M][ldx] (round 6: the LSTM bias gradients of the bf16 mode, reference model.py:352-371 under
 * autograd, from the gate-gradient slabs the weight-gradient products read).  N, ldx multiples of 8; sums in double. */
int t2amd_colsum_bf16(const void* x16, long long ldx, int M, int N, double* ws, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * small data-movement kernels (reference model.py:503 embedding, :296-309 / :326-336
 * parse_decoder_inputs/outputs, :487-497 parse_output).
 * ------------------------------------------------------------------------------------ */
int t2amd_embedding_fwd_f32(const long long* ids, const float* table, float* out, long long rows,
                            int dim, int n_symbols, void* stream);
/* dtable[s] = sum of the dout rows whose id is s, in a fixed order (eight interleaved row lanes, no atomics).  ws is unused (may be
 * NULL); it stays in the signature for callers built against the earlier partial-sum version. */
int t2amd_embedding_bwd_f32(const long long* ids, const float* dout, float* dtable, float* ws, long long rows,
                            int dim, int n_symbols, void* stream);
/* Philox4x32-10 keep-mask: out[i] = uniform(seed, offset+i) >= p */
int t2amd_philox_keep_mask(uint8_t* out, long long n, float p, unsigned long long seed,
                           unsigned long long offset, void* stream);
int t2amd_fill_f32(float* p, long long n, float v, void* stream);
/* dst[i] = bf16(src[i]) (round to nearest even); n % 4 == 0 */
int t2amd_cast_bf16_f32(const float* src, void* dst, long long n, void* stream);
/* Split-bf16 operand image (round 6, the 'bf16x3' mode of the LSTM tiles: t2amd_lstm_step.bf16 == 3).  src is f32 [rows][K]
 * (row stride lds floats), K % 16 == 0; dst takes 4 bytes per k (row stride ldd in k, ldd >= K): for every group of 16
 * consecutive k, 16 bf16 `hi = bf16(x)` followed by 16 bf16 `lo = bf16(x - hi)` (both round to nearest even), so that one
 * 64-byte group of a row feeds the 32x32x16 bf16 MFMA its hi and its lo fragment of the same 16 k.  x = hi + lo to ~2^-17. */
int t2amd_split_bf16x3_f32(const float* src, long long lds, void* dst, long long ldd, long long rows, int K, void* stream);
/* dst[r][c] = src[r][c] (+ src2[r][c] if src2) for r<rows, c<cols */
int t2amd_copy2d_f32(const float* src, long long lds, const float* src2, long long lds2, float* dst,
                     long long ldd, int rows, int cols, void* stream);
/* dst[c][r] = src[r][c], batched */
int t2amd_transpose_f32(const float* src, long long lds, float* dst, long long ldd, int rows,
                        int cols, int batch, long long sstride, long long dstride, void* stream);
/* teacher frames: mels [B][C][To] -> X0 [To][B][C] with X0[0]=0, X0[t]=mels[:,:,t-1] */
int t2amd_frames_to_time_major_f32(const float* mels, float* x0, int B, int C, int To, void* stream);
/* projection slab PG [To][B][C+1] -> mel_cl [B][To][C] (unmasked), gate [B][To] (1e3 where
 * t >= out_lens[b], if out_lens) */
int t2amd_split_projection_f32(const float* pg, float* mel_cl, float* gate, const int* out_lens,
                               int B, int C, int To, void* stream);
/* mel_cl,[post_cl] [B][To][C] -> mel,[mel_post = mel+post] [B][C][To], zeroed where t >= out_lens[b];
 * mel_cl itself is zeroed in place at padded frames (reference model.py:493: the in-place fill
 * reaches the tensor the first Postnet conv saved for backward). */
int t2amd_finalize_outputs_f32(float* mel_cl, const float* post_cl, float* mel, float* mel_post,
                               const int* out_lens, int B, int C, int To, void* stream);
/* backward entry: dmel,dmel_post [B][C][To] (either may be NULL) -> dpost_cl [B][To][C] = dmel_post^T,
 * dmel_cl [B][To][C] = dmel^T + dmel_post^T */
int t2amd_grads_to_channel_last_f32(const float* dmel, const float* dmel_post, float* dmel_cl,
                                    float* dpost_cl, int B, int C, int To, void* stream);
/* D_out [To][B][C+1] = [ dmel_cl[b][t][:] | dgate[b][t] ] */
int t2amd_gather_dout_f32(const float* dmel_cl, const float* dgate, float* dout, int B, int C,
                          int To, void* stream);
/* Prenet backward, elementwise part (reference model.py:99 F.dropout(F.relu(.)) under autograd):
 * dy <- (y > 0) ? dy*scale : 0, y being the forward output relu(pre)*keep*scale. */
int t2amd_relu_dropout_bwd_f32(float* dy, const float* y, float scale, long long n, void* stream);
/* alignments slab [B][To][Ti] passthrough needs no kernel. */

/* ------------------------------------------------------------------------------------
 * Recurrent cell kernels: batch x hidden "skinny" GEMM on v_mfma_f32_16x16x4_f32 with the
 * LSTM cell fused in the epilogue.  Replace torch.nn.LSTMCell / nn.LSTM + F.dropout at
 * reference model.py:352-356 (attention_rnn), :366-371 (decoder_rnn), :181-188 (encoder
 * bi-LSTM, packed-sequence semantics through `lens`/`t`).
 * ------------------------------------------------------------------------------------ */
typedef struct t2amd_seg {
    const float* p;  /* [B][width] rows, NULL = all zeros */
    long long ld;
    int width;       /* multiple of 64 */
} t2amd_seg;

typedef struct t2amd_lstm_step {
    t2amd_seg x[3];
    int nseg;
    const float* W;     /* [4H][Ktot], K contiguous, Ktot = sum widths; row g*H+j = gate g unit j */
    int Ktot, H, B;
    const float* gin;   /* [B][4H] pre-activation addend or NULL */
    long long ld_gin;
    const float* bias;  /* [4H] or NULL */
    const float* c_prev; /* [B][H] or NULL (zeros) */
    long long ld_cprev;
    float* gates_out;   /* [B][4H] activated gates i,f,g,o (may alias gin); NULL (round 6): not stored -- only a backward reads them */
    long long ld_gates;
    float* c_out;
    long long ld_c;
    float* h_out;       /* dropped-out hidden state */
    long long ld_h;
    const uint8_t* keep; /* [B][H] or NULL */
    long long ld_keep;
    float keep_scale;
    const int* lens;    /* NULL, or per-row valid length: rows with t >= lens[b] write h=c=gates=0 */
    int t;
    int tag;            /* kernel-symbol / profiling role: 0 generic, 1 attention LSTM, 2 decoder LSTM, 3 fused pair */
    /* bf16 operand mode: x[i].p and W point at bf16 (widths / ld / Ktot count ELEMENTS, widths multiples of 128);
     * the product runs on v_mfma_f32_16x16x32_bf16 with f32 accumulation; gin, bias, cell state and all f32
     * outputs are unchanged.  h16_out (optional) receives a bf16 copy of h, the next step's operand.
     * t2amd_lstm_step_small_f32 accepts 0 or 2: 2 = W alone is bf16, x[i].p stay f32 (matrix-vector path).
     * 3 (round 6, the engine's 'bf16x3' mode): x[i].p and W point at SPLIT-bf16 images (t2amd_split_bf16x3_f32: 4 bytes per k,
     * every 16 k as 16 hi then 16 lo bf16); widths / ld / Ktot count k as in the f32 form (widths multiples of 64); the
     * product is Xh.Wh + Xl.Wh + Xh.Wl on v_mfma_f32_32x32x16_bf16 with f32 accumulation (~2^-17 relative per product:
     * f32-class results at the f32 byte stream and 3/16 of the exact-f32 MFMA time); h16_out receives the split image of h
     * (ld_h16 in k). */
    int bf16;
    void* h16_out;
    long long ld_h16;
} t2amd_lstm_step;

int t2amd_lstm_step_fwd_f32(const t2amd_lstm_step* a, void* stream);
/* Two independent steps in ONE launch (b may be NULL): the time loops pair the decoder LSTM of step
 * t-1 with the attention LSTM of step t, neither depends on the other (reference model.py:352-371). */
int t2amd_lstm_step_fwd2_f32(const t2amd_lstm_step* a, const t2amd_lstm_step* b, void* stream);

/* Small-batch (B <= 8) variants for free-running decode (reference model.py:418-454 at B = 1, BASELINE
 * config 4): matrix-vector kernels bound by the weight stream instead of 64-row MFMA tiles. */
int t2amd_lstm_step_small_f32(const t2amd_lstm_step* a, void* stream);
typedef struct t2amd_small_linear {
    const float* X;      /* [B][ldx] */
    long long ldx;
    const float* W;      /* [N][ldw], K-contiguous (nn.Linear layout), 16-byte aligned rows */
    long long ldw;
    const float* bias;   /* [N] or NULL */
    float* Y;            /* [B][ldy] */
    long long ldy;
    int B, N, K;         /* B <= 8, K % 4 == 0 */
    int act;             /* 0 none, 1 relu */
    const uint8_t* keep; /* [B][ldkeep] or NULL */
    long long ldkeep;
    float keep_scale;
} t2amd_small_linear;
/* Y = act(X . W^T + bias) * keep * keep_scale   (Prenet linears model.py:99, projection + gate :373-378) */
int t2amd_linear_small_f32(const t2amd_small_linear* a, void* stream);

/* Y[s][B][N] = X[B][K-range s] . W[N][K]^T  (W K-contiguous), s < nsplit */
typedef struct t2amd_skinny_gemm {
    t2amd_seg x[3];
    int nseg;
    const float* W;   /* [N][Ktot] */
    int Ktot, N, B;
    float* Y;         /* [nsplit][B][ldy] */
    long long ldy;
    int nsplit;
    long long split_stride;
    int tag;          /* kernel-symbol role, as in t2amd_lstm_step */
    int bf16;         /* 1: x[i].p and W are bf16 (see t2amd_lstm_step) */
    /* optional epilogue (nsplit must be 1 when any of it is used): Y = keep ? act(Y + bias) * keep_scale : 0 --
     * nn.Linear + F.relu + F.dropout of the per-step prenet / projection at decode batch sizes 9..
     * (reference model.py:99, 373-378) */
    const float* bias;        /* [N] or NULL */
    int act;                  /* 0 none, 1 relu */
    const uint8_t* keep;      /* [B][ld_keep] keep mask or NULL */
    long long ld_keep;
    float keep_scale;
    void* Y16;                /* optional bf16 copy of Y (first split only), row stride ldy16 */
    long long ldy16;
    /* optional stop test of free-running decoding (reference model.py:439-444; nsplit must be 1), run by the thread that
     * holds the final value of column stop_col (the gate logit) of a row with stop_active[row] != 0:
     * sigmoid(Y) > stop_threshold (strict) or stop_t + 1 >= stop_max_steps  ->  stop_lengths[row] = stop_t + 1,
     * stop_active[row] = 0, ++*stop_done.  stop_active == NULL: no test. */
    uint8_t* stop_active;
    int* stop_lengths;
    int* stop_done;
    int stop_col, stop_t, stop_max_steps;
    float stop_threshold;
} t2amd_skinny_gemm;

int t2amd_skinny_gemm_f32(const t2amd_skinny_gemm* a, void* stream);
int t2amd_skinny_gemm2_f32(const t2amd_skinny_gemm* a, const t2amd_skinny_gemm* b, void* stream);

typedef struct t2amd_addend {
    const float* p;   /* NULL = absent */
    long long ld;
    int nsplit;       /* >=1 partial slabs summed */
    long long split_stride;
} t2amd_addend;

typedef struct t2amd_lstm_bwd {
    int B, H;
    t2amd_addend dh[3];   /* gradient wrt the dropped-out h, summed */
    const float* gates;   /* [B][4H] activated */
    long long ld_gates;
    const float* c_prev;  /* NULL = zeros */
    long long ld_cprev;
    const float* c;       /* [B][H] */
    long long ld_c;
    const uint8_t* keep;
    long long ld_keep;
    float keep_scale;
    float* dc;            /* [B][H] carry, in: dL/dc_t from step t+1, out: dL/dc_{t-1} */
    long long ld_dc;
    float* dgates;        /* [B][4H] out; may be NULL beside dgates16 (round 6): the operand copy is then the cell's only gate-gradient output */
    long long ld_dgates;
    const int* lens;
    int t;
    void* dgates16;       /* optional bf16 copy of dgates (bf16 operand mode of the dgrad GEMM) */
    long long ld_dgates16;
    int dgates16_x3;      /* 1: dgates16 receives the SPLIT-bf16 image of dgates instead (t2amd_split_bf16x3_f32 layout, ld_dgates16 in k) */
} t2amd_lstm_bwd;

int t2amd_lstm_pointwise_bwd_f32(const t2amd_lstm_bwd* a, void* stream);
int t2amd_lstm_pointwise_bwd2_f32(const t2amd_lstm_bwd* a, const t2amd_lstm_bwd* b, void* stream);

/* ------------------------------------------------------------------------------------
 * Location-sensitive attention, one decoder step (reference model.py:43-86 Attention.forward /
 * get_alignment_energies, :22-26 LocationLayer, :358-365 concat + cumulative update).
 * U[d][c*31+k] = sum_f Wdense[d][f]*Wconv[f][c][k] is the location conv and dense folded
 * into one 62-tap filter per attention dim (t2amd_fold_location_f32, U = 128*62 floats).
 * Each step is two launches of T2AMD_ATT_SLICES x B workgroups (energies over dim slices, then
 * softmax + context over channel slices); partial results cross between them through `ws`.
 * ------------------------------------------------------------------------------------ */
int t2amd_fold_location_f32(const float* wdense, const float* wconv, float* U, void* stream);
/* dWdense[d][f] = sum_ck dU[d][ck]*Wconv[f][ck]; dWconv[f][ck] = sum_d Wdense[d][f]*dU[d][ck];
 * dU = sum over nb per-utterance accumulators dU_acc[nb][128][62]; dv = sum_b dv_acc[nb][128] */
int t2amd_unfold_location_grads_f32(const float* dU_acc, const float* dv_acc, int nb,
                                    const float* wdense, const float* wconv, float* dwdense,
                                    float* dwconv, float* dv, void* stream);

typedef struct t2amd_attn_fwd {
    int B, Ti, E, Hq;        /* E = encoder dim (multiple of 16), Hq = attention_rnn_dim (multiple of 32) */
    const float* h;          /* [B][Hq] query source (dropped-out attention hidden), 16-byte aligned rows */
    long long ld_h;
    const float* Wq;         /* [128][Hq] query_layer weight, as stored by nn.Linear */
    const float* U;          /* [128][62] */
    const float* v;          /* [128] */
    const float* pm;         /* [B][Ti][128] processed memory */
    const float* memory;     /* [B][Ti][E] */
    const int* lens;         /* [B] or NULL (no mask: reference inference) */
    const float* w_prev;     /* previous weights, row b at w_prev + b*ld_wprev; NULL = zeros */
    long long ld_wprev;
    float* cum;              /* [B][Ti] running cumulative weights, updated in place */
    float* cum_save;         /* [B][Ti] copy of cum BEFORE the update, or NULL */
    float* w_out;            /* row b at w_out + b*ld_wout */
    long long ld_wout;
    float* ctx_out;          /* [B][E] */
    long long ld_ctx;
    float* q_out;            /* [B][128] or NULL */
    long long ld_q;
    const uint8_t* active;   /* [B] or NULL: rows with active[b]==0 are skipped (batched inference) */
    float* ws;               /* workspace, >= T2AMD_ATT_SLICES*B*Ti floats (partial energies) */
    void* ctx16_out;         /* optional bf16 copy of the context [B][ld_ctx16] (bf16 operand mode) */
    long long ld_ctx16;
    /* 1: the location convolution runs as a split-bf16 product (U = Uh + Ul, window = Wh + Wl in bf16;
     * Uh.Wh + Uh.Wl + Ul.Wh on v_mfma_f32_16x16x32_bf16, f32 accumulate: ~2^-17 relative per product) -- the
     * engine's bf16 compute mode.  0: exact-f32 MFMA (parity mode). */
    int loc_split_bf16;
    /* optional bf16 copy of `memory` ([B][Ti][E] bf16): the context product then streams it instead of the f32 rows
     * (the kernel is bound by the bytes of those rows); weights, accumulation and the context stay f32. */
    const void* memory16;
    /* optional bf16 copy of Wq ([128][Hq] bf16): the query product q = Wq h streams it (h and the sums stay f32) */
    const void* Wq16;
    /* Size of ws in floats, or 0 = "the minimum".  With at least t2amd_attn_fwd_ws_floats(B, Ti) floats -- the block
     * behind the partial energies zeroed once -- the step may run as ONE launch whose four workgroups per utterance hand
     * the partial energies to each other as 8-byte {launch token, value} granules (t2amd_set_attn_fwd_fused). */
    long long ws_floats;
    /* 1: ctx16_out receives the SPLIT-bf16 image of the context (t2amd_split_bf16x3_f32 layout, ld_ctx16 in k; E % 16 == 0) --
     * the operand of the 'bf16x3' LSTM tiles; everything else of the step stays in its exact-f32 form. */
    int ctx16_x3;
} t2amd_attn_fwd;

int t2amd_attention_step_fwd_f32(const t2amd_attn_fwd* a, void* stream);
/* floats of ws that every form of the call can use (a multiple of 4) */
long long t2amd_attn_fwd_ws_floats(int B, int Ti);
/* 1: K_e and K_c of a step run as one launch (energy granules between the four workgroups of an utterance), 0: two
 * launches, -1: library default / environment T2AMD_ATTN_FWD_FUSED.  Bit-identical results.  The one-launch form serves
 * launches of at most 512 workgroups (B <= 128) with Ti <= 512.  Its launch token is a kernel argument drawn from a
 * process-wide counter at enqueue time: do not capture these launches into a hipGraph (a replay would present the same
 * token again and accept the previous replay's granules); the same holds for the one-launch forms of the backward. */
int t2amd_set_attn_fwd_fused(int on);

typedef struct t2amd_attn_bwd {
    int B, Ti, E, Hq;
    t2amd_addend dctx[3];    /* gradient wrt the context vector, column offset pre-applied to p */
    float* dctx_total;       /* [B][E] out (saved for the deferred d_memory GEMM) */
    long long ld_dctx_total;
    const float* d_w_extra;  /* upstream grad wrt this step's weights (alignments output) or NULL */
    long long ld_dwextra;
    const float* q;          /* [B][128] saved */
    long long ld_q;
    const float* Wq;         /* [128][Hq] */
    const float* U;          /* [128][62] */
    const float* v;
    const float* pm;
    const float* memory;
    const int* lens;
    const float* w;          /* this step's weights, row stride ld_w */
    long long ld_w;
    const float* w_prev;     /* NULL = zeros */
    long long ld_wprev;
    const float* cum_before; /* [B][Ti] */
    /* Carries between steps, in partial form.  dwin_part[s][b][c][ti], s < T2AMD_ATT_SLICES, c = 0: grad
     * wrt the PREVIOUS weights (the next-processed step's w), c = 1: grad wrt the cumulative weights, both
     * from the location input of the step processed before this call.  In: partials of step t+1; out:
     * partials of this step.  dcum_acc[b][ti]: running gradient wrt the cumulative weights; on return it
     * includes the incoming c = 1 partials.  Zero both before the last time step. */
    float* dwin_part;        /* [T2AMD_ATT_SLICES][B][2][Ti] in/out */
    float* dcum_acc;         /* [B][Ti] in/out */
    float* d_pm;             /* [B][Ti][128] accumulated */
    float* dU_acc;           /* [B][128][62] accumulated */
    float* dv_acc;           /* [B][128] accumulated */
    float* dq_out;           /* [B][128] */
    long long ld_dq;
    float* dh_out;           /* [T2AMD_ATT_SLICES] partial slabs of Wq^T dq: slice s, row b at dh_out + s*dh_split_stride + b*ld_dh */
    long long ld_dh;
    long long dh_split_stride;
    float* ws;               /* workspace, >= B*Ti + 8*B floats (12*B with cell_q).  Words [B*Ti + 4*B, B*Ti + 8*B) (and
                              * the next 4*B with cell_q) receive the hand-off tokens of the fused kernel (a nonzero
                              * launch counter): zero them once before the first call and do not let other kernels
                              * write there between calls. */
    /* 1: the two gradient products of the location layer (dcol = U^T dpre, dU += dpre^T im2col) round their
     * operands to bf16 and run on v_mfma_f32_16x16x32_bf16 (f32 accumulate) -- the engine's bf16 compute mode.
     * 0: exact-f32 MFMA.  The recompute of the location conv uses the forward's split-bf16 form (see
     * t2amd_attn_fwd.loc_split_bf16) when this is 1, the exact-f32 MFMA otherwise.
     * 2 (round 6, the 'bf16x3' mode): the recompute in the split-bf16 form, the two gradient products exact f32. */
    int bf16;
    /* optional bf16 copy of `memory`: dw = dctx . memory streams it instead of the f32 rows */
    const void* memory16;
    /* Optional (both NULL = off): the LSTM cell backwards of a BPTT step (reference: nn.LSTMCell under autograd,
     * model.py:351-352, 366-370), run as the closing phase of THIS launch instead of a t2amd_lstm_pointwise_bwd2_f32
     * launch of their own.
     *   cell_q: the cell whose dL/dh contains this step's W_q^T dq -- the attention LSTM of the step.  Its dh[1] must
     *           describe dh_out's T2AMD_ATT_SLICES slabs (what a separate launch would read); H = Hq, same B.
     *   cell_x: a cell that does not depend on this launch (the decoder LSTM of step t-1), or NULL.
     * In the folded form the four workgroups of an utterance exchange their dq slices through dq_out behind a second
     * token block (ws must then hold B*Ti + 12*B floats, the last 8*B zeroed once), each forms W_q^T dq for a quarter
     * of the columns in the summation order of the dh_out slabs, and runs both cells for those units: results are
     * bit-identical to the separate launch; dh_out is not written.  Geometries the folded form does not cover
     * (Hq % 16 != 0, H > 1024, the two-launch form of this step) run the cells as a separate launch from inside the
     * call. */
    const t2amd_lstm_bwd* cell_q;
    const t2amd_lstm_bwd* cell_x;
    /* Size of ws in floats, or 0 = "the minimum".  With at least t2amd_attn_bwd_ws_floats(B, Ti) floats (zeroed once from
     * word B*Ti on) the first hand-off of the one-launch form may travel as 8-byte {launch token, value} granules in the
     * block behind the token words (t2amd_set_attn_bwd_granules). */
    long long ws_floats;
    /* optional bf16 copy of Wq ([128][Hq] bf16, 16-byte aligned, Hq % 8 == 0): the closing product dh = Wq^T dq streams it instead
     * of the f32 rows (dq and the sums stay f32) -- the engine's bf16 compute mode; the folded and the separate-launch forms
     * read the same copy in the same order and stay bit-identical to each other. */
    const void* Wq16;
} t2amd_attn_bwd;

int t2amd_attention_step_bwd_f32(const t2amd_attn_bwd* a, void* stream);
/* floats of ws that every form of the call can use: dw slab, slice partials, two token blocks, granule block */
long long t2amd_attn_bwd_ws_floats(int B, int Ti);
/* First hand-off of the one-launch form (dw slices between the four workgroups of an utterance): 1 = 8-byte
 * {token, value} granules polled by their consumers, 0 = write-through stores + drain + token + payload loads,
 * -1 = library default / environment T2AMD_ATTN_GRANULES.  Bit-identical results. */
int t2amd_set_attn_bwd_granules(int on);
/* Number of in-launch hand-offs of the one-launch attention forms that were ABANDONED since the last reset (their bounded
 * 50 ms spin ran out: the workgroups of an utterance were not co-resident, e.g. a shared or partitioned GPU).  Such a
 * launch poisons its outputs with NaN; a caller that finds a non-finite loss / gradient norm asks here whether that is
 * the reason and, if so, selects the separate-launch forms (t2amd_set_attn_fwd_fused(0), T2AMD_ATTN_FUSED_BWD=0 /
 * t2amd_set_attn_bwd_fused(0)).  Synchronises with the device; -1 on error. */
int t2amd_attn_handoff_timeouts(int reset);
/* 0: the attention backward of a step as two launches (K_b1, K_b2; no in-launch hand-off, the LSTM cell backwards in
 * their own launch); 1: one launch (default); -1: the T2AMD_ATTN_FUSED_BWD environment default */
int t2amd_set_attn_bwd_fused(int on);

/* ------------------------------------------------------------------------------------
 * Device-resident time loops.  One host call enqueues every step's kernels.
 * ------------------------------------------------------------------------------------ */
/* Teacher-forced decoder loop, forward: reference model.py:405-411 (the while loop) around
 * Decoder.decode :340-379.  Prenet, input projection, memory_layer and the mel/gate
 * projection are hoisted out of the loop by the host (dense GEMMs over all steps). */
typedef struct t2amd_dec_train {
    int B, Ti, To, E, Ha, Hd;
    /* weights */
    const float* Wa_rec;   /* [4Ha][E+Ha] = [W_ih_att[:, P:P+E] | W_hh_att] */
    const float* Wd_cat;   /* [4Hd][Ha+E+Hd] = [W_ih_dec | W_hh_dec] */
    const float* bias_d;   /* [4Hd] = b_ih + b_hh */
    const float* Wq;       /* [128][Ha] */
    const float* U;        /* [128][62] */
    const float* v;        /* [128] */
    /* inputs */
    float* GA;             /* [To][B][4Ha] in: prenet input projection + att biases; out: activated gates */
    const float* memory;   /* [B][Ti][E] */
    const float* pm;       /* [B][Ti][128] */
    const int* lens;       /* [B] */
    const uint8_t* keep_att; /* [To][B][Ha] */
    const uint8_t* keep_dec; /* [To][B][Hd] */
    float scale_att, scale_dec;
    /* saved slabs (outputs) */
    float* HA;  /* [To][B][Ha] */
    float* CA;  /* [To][B][Ha] */
    float* GD;  /* [To][B][4Hd] */
    float* HD;  /* [To][B][Hd] */
    float* CD;  /* [To][B][Hd] */
    float* CTX; /* [To][B][E] */
    float* Q;   /* [To][B][128] */
    float* ALIGN; /* [B][To][Ti] */
    float* CUM;   /* [To][B][Ti] cumulative weights before each step */
    float* cum_work; /* [B][Ti] scratch (zeroed by the call) */
    float* attn_ws;  /* >= T2AMD_ATT_SLICES*B*Ti + B*Ti + 8*B floats: attention workspace (the backward loop uses the
                      * part behind the forward's T2AMD_ATT_SLICES*B*Ti) */
    /* bf16 operand mode (all NULL / 0 for f32): bf16 copies of the packed weights and of the three recurrent
     * operand slabs; the LSTM products then run on the bf16 MFMA, state and slabs above stay f32. */
    int bf16;
    const void* Wa_rec16;  /* [4Ha][E+Ha] bf16 */
    const void* Wd_cat16;  /* [4Hd][Ha+E+Hd] bf16 */
    void* HA16;            /* [To][B][Ha] bf16 */
    void* HD16;            /* [To][B][Hd] bf16 */
    void* CTX16;           /* [To][B][E] bf16 */
    const void* memory16;  /* [B][Ti][E] bf16 copy of memory, or NULL: attention context / its backward stream it */
    const void* Wq16;      /* [128][Ha] bf16 copy of Wq, or NULL: the forward query product streams it */
} t2amd_dec_train;

int t2amd_decoder_train_fwd_loop_f32(const t2amd_dec_train* p, void* stream);

/* The same loop as ONE persistent launch (reference model.py:405-411 around Decoder.decode :340-379; BASELINE north_star:
 * "the decode loop is fused into a persistent wavefront-resident kernel").  max(Ha/8 + Hd/8, 4 B) co-resident 512-thread
 * workgroups alternate the LSTM-tile role and the attention role of every time step; the two all-to-all edges of a step are
 * flag + data hand-offs (write-through payload, one step counter per workgroup in `flags`:
 * t2amd_decoder_train_fwd_persistent_flag_bytes(B, Ha) bytes, zeroed by the call).  Same arithmetic in the same order as the
 * launch chain above: every output is bit-identical to it.  Both operand modes since round 5: p->bf16 with every bf16 copy
 * present (bf16 MFMA tiles, bf16 attention streams), or p->bf16 == 0 -- the fp32 parity mode: the same loop over the f32 slabs,
 * tiles on the exact-f32 MFMA, which the chain above then runs as well.  Inside the launch a workgroup fetches the first four
 * k-tiles of its NEXT LSTM tile while it sits in its attention step (T2AMD_DTP_PREFETCH=0 switches that off).
 * B <= 64, Ti <= 512; `_supported` returns 0 when the geometry fits a device of `cus` compute units (every workgroup must be
 * resident at once), else T2AMD_ERR_ARG with the reason in t2amd_last_error().  Spins are bounded (50 ms of the wall clock):
 * a give-up sets *status != 0 and every workgroup leaves; with `poison` non-NULL a one-thread launch behind the kernel
 * turns poison[0] into NaN in that case (for callers that do not read status back) and counts it for
 * t2amd_attn_handoff_timeouts(). */
long long t2amd_decoder_train_fwd_persistent_flag_bytes(int B, int Ha);
int t2amd_decoder_train_fwd_persistent_supported(const t2amd_dec_train* p, int cus);
int t2amd_decoder_train_fwd_persistent_f32(const t2amd_dec_train* p, unsigned* flags, int* status, float* poison, void* stream);

/* BPTT through the same loop (what autograd replays for reference train.py:226). */
typedef struct t2amd_dec_train_bwd {
    t2amd_dec_train f;       /* the forward description (slabs now inputs) */
    const float* Wa_recT;    /* [E+Ha][4Ha] */
    const float* Wd_catT;    /* [Ha+E+Hd][4Hd] */
    const float* DHC;        /* [To][B][Hd+E] grad wrt [h_dec | ctx] from the projection */
    const float* d_align;    /* [B][To][Ti] or NULL */
    int nsplit;              /* split-K factor of the two backward skinny GEMMs */
    /* outputs */
    float* DGA;  /* [To][B][4Ha] */
    float* DGD;  /* [To][B][4Hd]; round 6: DGA and DGD may both be NULL in the bf16 mode when DGA16 / DGD16 below are whole-sequence
                  * slabs (dg16_step_* > 0): nothing downstream reads the f32 slabs then (weight and bias gradients come from the
                  * bf16 slabs, t2amd_gemm16_kk_group / t2amd_colsum_bf16) and the cells stop writing them -- 2 MB per time step */
    float* DCTX; /* [To][B][E] */
    float* DQ;   /* [To][B][128] */
    float* d_pm; /* [B][Ti][128] (zeroed by the call) */
    float* dU_acc; /* [B][128][62] (zeroed by the call) */
    float* dv_acc; /* [B][128] (zeroed by the call) */
    /* workspaces */
    float* dXd;  /* [To][nsplit][B][Ha+E+Hd]: per step, the decoder-LSTM chain runs ahead of its consumers */
    float* dXa;  /* [nsplit][B][E+Ha] */
    float* dc_a; /* [B][Ha] */
    float* dc_d; /* [B][Hd] */
    float* dwin_part;  /* [T2AMD_ATT_SLICES][B][2][Ti] (zeroed by the call) */
    float* dcum_acc;   /* [B][Ti] (zeroed by the call) */
    float* dq_h;       /* [T2AMD_ATT_SLICES][B][Ha] */
    /* bf16 operand mode (f.bf16 != 0) */
    const void* Wa_recT16; /* [E+Ha][4Ha] bf16 */
    const void* Wd_catT16; /* [Ha+E+Hd][4Hd] bf16 */
    void* DGA16;           /* [B][4Ha] bf16 scratch: this step's attention-LSTM gate gradients */
    void* DGD16;           /* [B][4Hd] bf16 scratch */
    /* 0: DGA16 / DGD16 are one step's scratch, reused by every step; B*4Ha / B*4Hd: they are [To][B][4H] slabs and step t
     * writes (and its dgrad reads) its own rows -- the engine then builds the weight-gradient operands from them */
    long long dg16_step_a, dg16_step_d;
    /* (round 6) 0: dXd holds To step slabs (needed when the decoder-LSTM chain runs ahead on its own stream,
     * t2amd_set_decoder_streams(2)); R >= 3: dXd holds R step slabs used as a ring (step t -> slab t % R) -- a slab is read
     * one step after it is written and never again, and a ring stays in L2 / MALL instead of streaming To slabs to HBM.
     * Single-stream loop only. */
    int dXd_ring;
} t2amd_dec_train_bwd;

int t2amd_decoder_train_bwd_loop_f32(const t2amd_dec_train_bwd* p, void* stream);

/* (Round 6: the BPTT loop as ONE persistent launch -- t2amd_decoder_train_bwd_persistent_f32 and its _supported / _flag_bytes /
 * _desc_bytes queries, opt-in since round 4 -- was removed: two rounds at 1 ms behind the chain above, profiles/r04_j_ab_train_bwd_
 * persistent.json) */
/* 1 (default): everything on the caller's stream; the decoder-LSTM chain (off the attention recurrence under
 * teacher forcing) shares fused launches with the attention-LSTM chain.  2: the decoder-LSTM chain of both
 * training loops runs on an internal side stream, ordered against the caller's stream with one hipEvent per
 * 8 steps. */
int t2amd_set_decoder_streams(int n);
/* 1: the two LSTM cell backwards of a decoder BPTT step (attention LSTM of step t, decoder LSTM of step t-1) run as the
 * closing phase of the step's attention-backward launch (t2amd_attn_bwd.cell_q / cell_x): 5 dependent launches per
 * decoder time step instead of 6.  0: a launch of their own.  Gradients are bit-identical either way.  Start-up value:
 * environment T2AMD_CELL_FOLD, else the library default.  Single-stream loop only (t2amd_set_decoder_streams(1)). */
int t2amd_set_bptt_cell_fold(int on);
int t2amd_get_bptt_cell_fold(void);   /* the current value (0 / 1) */
/* Free-running decoder (t2amd_decoder_infer_steps_f32, reference model.py:418-454): the largest batch served by the matrix-vector
 * kernels; above it the step runs on the 64-row MFMA tiles, whose cost does not depend on B <= 64.  -1 (default): by operand mode
 * -- 3 rows with bf16 operands (t2amd_dec_infer.bf16 == 1), 4 otherwise (measured: profiles/r06_s_bench_infer_small_batches.txt);
 * 0 .. 8: that many rows (the matrix-vector kernels hold at most 8; 0 = tiles at every B).  Start-up value: environment
 * T2AMD_SMALL_BATCH_MAX.  A caller that sets up t2amd_dec_infer asks t2amd_dec_infer_uses_tiles (below) to know which operand copies the descriptor needs (bf16 / split-bf16 images and the folded prenet matrix Wf on the tile
 * path); bf16 == 3 with B at or below the boundary is refused (the split images belong to the tiles: pass 0 there). */
int t2amd_set_small_batch_max(int n);
int t2amd_get_small_batch_max(int bf16);
/* 1 when t2amd_decoder_infer_steps_f32 runs a batch of B rows in operand mode `bf16` on the tiles, 0 for the matrix-vector kernels:
 * B above the boundary -- except that bf16 operands on widths that are not multiples of 128 (which the bf16 tiles refuse) stay on
 * the matrix-vector kernels up to their limit of 8 rows.  What a caller asks before it fills t2amd_dec_infer. */
int t2amd_dec_infer_uses_tiles(int B, int bf16, int E, int Ha, int Hd, int P);

/* Encoder bi-LSTM over [B][T][.] with packed-sequence semantics (reference model.py:180-188).
 * GX [B][T][4H] holds x.W_ih^T + b_ih + b_hh (hoisted dense GEMM) and is overwritten with the
 * activated gates.  out: [B][T][ld_out] slice (direction offset pre-applied). */
typedef struct t2amd_lstm_seq {
    int B, T, H, reverse;
    const float* Whh;   /* [4H][H] */
    const float* WhhT;  /* [H][4H] (backward only) */
    float* GX;          /* [B][T][4H] */
    float* out;         /* h outputs, element (b,t,j) at out[(b*T+t)*ld_out + j] */
    long long ld_out;
    float* C;           /* [T][B][H] cell states */
    const int* lens;
    /* backward only */
    const float* dout;  /* grad wrt out, same indexing with ld_dout */
    long long ld_dout;
    float* DG;          /* [B][T][4H] out: gate pre-activation grads */
    float* dX;          /* [max(dx_splits, 1)][B][H] workspace */
    float* dc;          /* [B][H] workspace */
    /* backward: 2..4 = the recurrent data-gradient product dh_prev = dgates . Whh of every step splits its K = 4H over
     * that many groups of workgroups, which write partial slabs of dX that the next step's cell backward adds in index
     * order (H/16 column tiles alone are 16 workgroups per direction at H = 256: a 16-tile dependent k loop on a
     * handful of CUs).  0 / 1: one slab. */
    int dx_splits;
} t2amd_lstm_seq;

int t2amd_lstm_seq_fwd_f32(const t2amd_lstm_seq* p, void* stream);
int t2amd_lstm_seq_bwd_f32(const t2amd_lstm_seq* p, void* stream);
/* Both directions of the bi-LSTM in lockstep, one launch per step for the pair (q may be NULL). */
int t2amd_lstm_seq_fwd2_f32(const t2amd_lstm_seq* p, const t2amd_lstm_seq* q, void* stream);
int t2amd_lstm_seq_bwd2_f32(const t2amd_lstm_seq* p, const t2amd_lstm_seq* q, void* stream);
/* The same forward recurrence for ONE utterance (B == 1, H <= 256; Encoder.inference, reference model.py:192-201) as ONE
 * persistent launch of 2 x H/4 co-resident workgroups: W_hh rows in registers, h exchanged as {step + 1, f32} granules in
 * `mailbox` (t2amd_lstm_seq_persistent_mailbox_bytes(H, ndir) bytes, zeroed by the call).  Inference only: writes `out`,
 * leaves GX / C untouched.  Bounded spins: *status != 0 afterwards = a workgroup gave up, run t2amd_lstm_seq_fwd2_f32. */
long long t2amd_lstm_seq_persistent_mailbox_bytes(int H, int ndir);
int t2amd_lstm_seq_persistent_supported(const t2amd_lstm_seq* p);
int t2amd_lstm_seq_fwd2_persistent_f32(const t2amd_lstm_seq* p, const t2amd_lstm_seq* q, unsigned long long* mailbox,
                                       int* status, void* stream);
/* The same recurrence for a BATCH (B > 1: the training forward, batched inference) as ONE persistent launch of
 * ndir x ceil(B / 32) x H/4 co-resident workgroups: each keeps its 16 gate rows of W_hh in registers as exact-f32 MFMA
 * fragments and the cell state of its 32 x 4 cells; h(s) is handed on through the output slab itself (write-through stores,
 * one step counter per workgroup in `flags` -- t2amd_lstm_seq_batch_persistent_flag_bytes(B, H, ndir) bytes, zeroed by the
 * call -- polled by the H/4 workgroups of the same direction and row group).  Writes everything the launch chain writes
 * (out, C, GX overwritten with the activated gates): the backward is unchanged.  Exact f32 like t2amd_lstm_seq_fwd2_f32 (other
 * summation order: ~2e-7).  Bounded spins: *status != 0 afterwards = a workgroup gave up (GPU shared?): recompute GX and run
 * t2amd_lstm_seq_fwd2_f32.  `cus` = the device's CU count (at most 4 workgroups per CU are assumed co-resident).
 * `poison` (may be NULL): for callers that do not read `status` back -- the training step, where a host sync per step would
 * tie the step time to the host's enqueue speed -- a give-up writes NaN to *poison behind the launch (the step goes non-finite
 * and is skipped like an abandoned attention hand-off) and t2amd_encoder_handoff_timeouts() counts it. */
long long t2amd_lstm_seq_batch_persistent_flag_bytes(int B, int H, int ndir);
int t2amd_lstm_seq_batch_persistent_supported(const t2amd_lstm_seq* p, int ndir, int cus);
int t2amd_lstm_seq_fwd2_batch_persistent_f32(const t2amd_lstm_seq* p, const t2amd_lstm_seq* q, unsigned* flags, int* status,
                                             float* poison, void* stream);
/* BPTT of the same recurrence for a batch as ONE persistent launch (reference model.py:181-188 under autograd) instead of
 * 2 T dependent launches (t2amd_lstm_seq_bwd2_f32): same workgroup layout, flag buffer size and hand-off as the forward launch
 * above; the gate gradients go straight into p->DG (the slab the weight-gradient GEMMs read), the recurrent data gradient is a
 * split-bf16 (hi + lo, three products, f32 accumulate: ~2^-17 relative) MFMA product against W_hh^T rows held in registers.
 * Reads WhhT, GX (activated gates), C, lens, dout; dX / dc of the descriptor are not used.  Results equal the chain's to that
 * product's rounding.  `_supported` / status / poison as for the forward launch. */
int t2amd_lstm_seq_bwd2_batch_persistent_supported(const t2amd_lstm_seq* p, int ndir, int cus);
int t2amd_lstm_seq_bwd2_batch_persistent_f32(const t2amd_lstm_seq* p, const t2amd_lstm_seq* q, unsigned* flags, int* status,
                                             float* poison, void* stream);
/* give-ups of that launch since the last reset (synchronises the device); negative on a runtime error */
int t2amd_encoder_handoff_timeouts(int reset);

/* Free-running decoder (reference model.py:418-454 Decoder.inference), any B: per-utterance
 * stop flags on the device, stop test sigmoid(gate) > threshold (strict) after the frame is
 * emitted.  Runs `n_steps` steps starting at step `t0` (host polls `done_count` between calls). */
typedef struct t2amd_dec_infer {
    int B, Ti, E, Ha, Hd, P, C;   /* P = prenet dim, C = n_mel_channels */
    int t0, n_steps, max_steps;
    float gate_threshold;
    const float* W1;       /* prenet layer 0 [P][C] */
    const float* W2;       /* prenet layer 1 [P][P] */
    const float* Wa_cat;   /* [4Ha][P+E+Ha] = [W_ih_att | W_hh_att] */
    const float* bias_a;   /* [4Ha] */
    const float* Wd_cat;   /* [4Hd][Ha+E+Hd] */
    const float* bias_d;
    const float* Wq;       /* [128][Ha] */
    const float* U;
    const float* v;
    const float* Wpg;      /* [C+1][Hd+E] = [linear_projection ; gate_layer] rows */
    const float* bias_pg;  /* [C+1] */
    const float* memory;
    const float* pm;
    const int* lens;       /* NULL = unmasked (reference B==1 path) */
    const uint8_t* keep_prenet; /* [max_steps][2][B][P] */
    /* state (persist across calls; zeroed by the caller before t0 == 0) */
    float* h_a;            /* [2][B][Ha] ping-pong: step t reads slot t&1, writes slot (t+1)&1 */
    float* c_a;            /* [2][B][Ha] */
    float* c_d;            /* [2][B][Hd] */
    float* hc;             /* [2][B][Hd+E] = [h_dec | ctx] ping-pong */
    float* cum;            /* [B][Ti] */
    float* x_prenet;       /* [2][B][P] scratch */
    float* gates;          /* unused since round 6 (was: [B][4*max(Ha,Hd)] scratch for gate activations nobody read; may be NULL) */
    const float* zero_frame; /* [B][C] zeros (go frame) */
    float* attn_ws;        /* >= T2AMD_ATT_SLICES*B*Ti floats */
    /* outputs */
    float* PG;             /* [max_steps][B][C+1] mel frame + gate logit per step */
    float* ALIGN;          /* [B][max_steps][Ti] */
    int* out_lengths;      /* [B] frames emitted incl. the stopping frame (0 while running) */
    uint8_t* active;       /* [B] 1 while the utterance is still decoding */
    int* done_count;       /* [1] number of finished utterances */
    /* bf16 operand mode for the two LSTM products (all NULL / 0 for f32): bf16 copies of the packed weights and,
     * for B > M (MFMA tile path; M = t2amd_get_small_batch_max(bf16): 3 with bf16 operands, 4 otherwise, unless set), of the recurrent operands, written by their producers next to the f32 values; the
     * matrix-vector kernels of B <= M read the bf16 weight rows against f32 inputs.  State, gates, attention and
     * outputs stay f32. */
    /* (3, round 6, B > M only: the 'bf16x3' mode -- Wa_cat16 / Wd_cat16 / x_prenet16 / h_a16 / hc16 are SPLIT-bf16 images
     * (t2amd_split_bf16x3_f32: two bf16 per k), the two LSTM steps run on the wide tile's split form; the optional pointers below
     * stay NULL: prenet, projection and attention keep their f32 operands) */
    int bf16;
    const void* Wa_cat16;  /* [4Ha][P+E+Ha] bf16 */
    const void* Wd_cat16;  /* [4Hd][Ha+E+Hd] bf16 */
    void* x_prenet16;      /* [B][P] bf16: prenet output of the current step */
    void* h_a16;           /* [2][B][Ha] bf16 ping-pong (zeroed before t0 == 0) */
    void* hc16;            /* [2][B][Hd+E] bf16 ping-pong (zeroed before t0 == 0) */
    /* B > M, optional: prenet layer 0 folded through the frame projection, Wf = W1 . Wp [P][Hd+E], bias_f = W1 . bp [P]
     * (p1 = relu(W1 (Wp hc + bp)) = relu(Wf hc + bias_f)): layer 0 of step t+1 then rides in step t's projection launch
     * instead of being a B x 256 x 80 tiled GEMM of its own.  NULL: the unfolded form. */
    const float* Wf;
    const float* bias_f;
    /* bf16 mode, B > M, optional: bf16 copies of the encoder memory [B][Ti][E] and of W_q [128][Ha] for the attention
     * kernels (they are bound by those streams); NULL: the f32 arrays are read. */
    const void* memory16;
    const void* Wq16;
    /* bf16 mode, B > M, optional (all four or none): bf16 copies of Wf [P][Hd+E], Wpg [C+1][Hd+E] and W2 [P][P] and a
     * [B][P] bf16 buffer for prenet layer 0's output -- the per-step prenet and frame/gate projection then run on the
     * bf16 MFMA path from the bf16 state copies the LSTM / attention kernels already write (f32 accumulation, f32
     * outputs; as the training loop's bf16 mode computes them) */
    const void* Wf16;
    const void* Wpg16;
    const void* W2_16;
    void* x_prenet1_16;
    /* floats in attn_ws, or 0 = "the minimum".  With t2amd_attn_fwd_ws_floats(B, Ti) floats, zeroed by the caller before the
     * first call, the attention step of launches of at most 512 workgroups runs as ONE launch (t2amd_attn_fwd.ws_floats). */
    long long attn_ws_floats;
} t2amd_dec_infer;

int t2amd_decoder_infer_steps_f32(const t2amd_dec_infer* p, void* stream);

/* Persistent, weight-stationary decode loop for ONE utterance (reference model.py:435-449 Decoder.inference's loop
 * around Decoder.decode :340-379; Prenet :97-100; Attention :43-86; LocationLayer :22-26): ONE launch of H/4
 * co-resident workgroups runs every step until the gate fires or max_steps is reached.  Each workgroup keeps its 16 rows
 * of both LSTM matrices (bf16 in LDS, or f32 split between LDS and registers: weights_f32) for the whole utterance; the six per-step vectors (p2, h_att, partial energies,
 * context, h_dec, p1 + stop flag) travel between workgroups as 8-byte {step + 1, f32} granules (agent-scope relaxed
 * stores / polled loads, no fences).  Prenet layer 0 is folded through the frame projection (Wf below).  Requires
 * attention_rnn_dim == decoder_rnn_dim = H, H/4 <= number of CUs, Ti <= 256 (t2amd_decoder_persist_supported).  Spins
 * are bounded (30 ms): on a timeout *status = T2AMD_PERSIST_TIMEOUT, every workgroup leaves and the caller must use
 * t2amd_decoder_infer_steps_f32 instead. */
#define T2AMD_PERSIST_TIMEOUT 7
typedef struct t2amd_dec_persist {
    int Ti, E, H, P, C;
    int max_steps;
    float gate_threshold;
    const void* Wa16;      /* [4H][P+E+H] bf16 = [W_ih_att | W_hh_att] */
    const void* Wd16;      /* [4H][H+E+H] bf16 = [W_ih_dec | W_hh_dec] */
    const float* bias_a;   /* [4H] b_ih + b_hh */
    const float* bias_d;   /* [4H] */
    const float* Wq;       /* [128][H] */
    const float* U;        /* [128][62] folded location filter (t2amd_fold_location_f32) */
    const float* v;        /* [128] */
    const float* Wf;       /* [P + C + 1][H+E]: rows 0..P-1 = W_prenet0 . W_proj, rows P..P+C-1 = W_proj, row P+C = W_gate */
    const float* bias_f;   /* [P + C + 1]: W_prenet0 . b_proj, b_proj, b_gate */
    const float* W2;       /* [P][P] prenet layer 1 */
    const float* memory;   /* [Ti][E] encoder outputs */
    const float* pm;       /* [Ti][128] processed memory */
    const uint8_t* keep_prenet; /* [max_steps][2][1][P] */
    float* PG;             /* [max_steps][C+1] frame + gate logit per step */
    float* ALIGN;          /* [max_steps][Ti] */
    int* out_length;       /* [1] frames emitted incl. the stopping frame */
    int* status;           /* [1] 0 = ok */
    int* steps_done;       /* [1] */
    unsigned long long* mailbox;  /* t2amd_decoder_persist_mailbox_bytes() bytes, zeroed by the call */
    float* trace;          /* NULL, or [max_steps][H + E + H + P + P]: h_att, ctx, h_dec, p1(t+1), p2(t+1) per step (tests) */
    unsigned long long* timing; /* NULL, or [32] zeroed by the caller: 100 MHz ticks per phase, summed over the steps, of
                                 * thread 0 of the first ([0..15]) and of the last ([16..31]) workgroup (tools) */
    int weights_f32;       /* 0: Wa16 / Wd16 are bf16 (throughput mode).  1: they point at the SAME matrices in f32 (the fp32
                            * parity mode: exact f32 products, the arithmetic of the fp32 launch chain): a workgroup then
                            * keeps its 16 attention-LSTM rows in LDS (16 x 1792 x 4 = 112 KB) and its 16 decoder-LSTM rows in
                            * REGISTERS (160 per lane: the CU's 512 KB register file holds what its 160 KB of LDS cannot);
                            * needs H and E multiples of 256 */
} t2amd_dec_persist;

long long t2amd_decoder_persist_mailbox_bytes(int Ti, int E, int H, int P);
int t2amd_decoder_persist_supported(const t2amd_dec_persist* p);
int t2amd_decoder_infer_persistent_f32(const t2amd_dec_persist* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Mel front end: element passes around the two GEMMs of
 * TacotronSTFT.mel_spectrogram (reference layers.py:63-80, stft.py:77-105,
 * audio_processing.py:78-84).  The contractions themselves are t2amd_gemm_f32 calls:
 *   spec[n][2F] = frames . basis^T with frames = the padded signal viewed as [n][L] with
 *   row stride hop (lda = hop < K: overlapping rows, no frame matrix), then
 *   mel[n][n_mel] = mag[n][Fpad] . mel_basis[n_mel][Fpad]^T.
 * ------------------------------------------------------------------------------------ */
/* out[b][i] = y[b][reflect(i - pad)] for i < T + 2*pad (torch 'reflect': the edge sample is not repeated;
 * needs pad < T), 0 for T + 2*pad <= i < Tout (row slack so that ldo can be a multiple of 4). */
int t2amd_reflect_pad_f32(const float* y, long long ldy, float* out, long long ldo, int B, int T, int pad,
                          int Tout, void* stream);
/* The index rule of the kernel above, callable on the host: position in y[0..T) of offset i in [-T+1, 2T-2]. */
long long t2amd_reflect_index(long long i, long long T);
/* mag[r][f] = sqrt(spec[r][f]^2 + spec[r][F+f]^2) for f < F, 0 for F <= f < Fpad; rows <= 65535 per call. */
int t2amd_stft_magnitude_f32(const float* spec, long long lds, float* mag, long long ldm, long long rows,
                             int F, int Fpad, void* stream);
/* out[b][m][j] = log(max(mel[(b*n + j)*ld + m], clip)): dynamic range compression + (frame, channel) transpose
 * into the (B, n_mel, n) layout TextMelCollate pads. */
int t2amd_mel_log_compress_f32(const float* mel, long long ld, float* out, int B, int n, int n_mel,
                               float clip, void* stream);

/* ------------------------------------------------------------------------------------
 * Mel front end, backward (csrc/audio_bwd.hip): the row passes between the two products of the way back,
 *   d_mag[R][Fpad] = d_mel[R][n_mel] . mel_basis and d_frames[R][L] = d_spec[R][Kp] . forward_basis
 * (t2amd_gemm_f32, precision 0 or 1), and a masked L1 loss on the log-mels.  The reference has no counterpart
 * (torch autograd differentiates layers.py:63-80 there).  No atomics: two calls give the same bits.
 * ------------------------------------------------------------------------------------ */
/* d_mel[(b*n + j)*ldd + m] = d_out[b][m][j] / mel[(b*n + j)*ld + m] where mel >= clip (the gradient passes at equality, torch's
 * clamp(min=) rule), exactly 0 elsewhere: t2amd_mel_log_compress_f32's gradient with its transpose undone. */
int t2amd_mel_log_bwd_f32(const float* d_out, const float* mel, long long ld, float* d_mel, long long ldd, int B, int n,
                          int n_mel, float clip, void* stream);
/* d_spec[r] = [d_mag re / mag (F) | d_mag im / mag (F) | 0 (Kp - 2F)] from spec[r] = [re (F) | im (F)]; mag is recomputed as
 * t2amd_stft_magnitude_f32 computes it; both gradients are exactly 0 where mag == 0 (a definition; torch's sqrt gives NaN). */
int t2amd_stft_magnitude_bwd_f32(const float* d_mag, long long ldm, const float* spec, long long lds, float* d_spec,
                                 long long ldd, long long rows, int F, int Kp, void* stream);
/* d_y[b][t] = the sum, in ascending padded position and ascending frame order, of d_frames[b*n + j][q - j*hop] over the padded
 * positions q that t2amd_reflect_index maps onto t (pad - t, pad + t, pad + 2(T-1) - t) and the frames j < n = T/hop + 1 that
 * cover q: the gradient of the strided frame view of t2amd_reflect_pad_f32's output, without a padded buffer. */
int t2amd_stft_frames_fold_f32(const float* d_frames, long long ldf, long long f_floats, float* d_y, long long ldy,
                               long long y_floats, int B, int T, int n, int L, int hop, int pad, void* stream);
/* (b, m) rows of n frames per partial slot of t2amd_mel_l1_fwd_f32. */
int t2amd_mel_l1_rows_per_slot(int n);
/* partial[s] = (sum over slot s's rows (b, m) and frames i < lens[b] of |out[b][m][i] - target[b][m][i]|) / count; out (B, n_mel, n),
 * target (B, n_mel, N), N <= n, lens NULL: N frames each; count = n_mel * sum(lens).  t2amd_wg_partial_sum_f32 over the
 * ceil(B n_mel / rows_per_slot) slots gives the loss. */
int t2amd_mel_l1_fwd_f32(const float* out, const float* target, const int* lens, int B, int n_mel, int n, int N,
                         long long count, float* partial, long long partial_floats, void* stream);
/* d_out[b][m][j] = sign(out - target) g[0] / count for j < lens[b], exactly 0 for the other j < n; g: the upstream scalar on the
 * device. */
int t2amd_mel_l1_bwd_f32(const float* out, const float* target, const int* lens, const float* g, int B, int n_mel, int n,
                         int N, long long count, float* d_out, void* stream);

/* Multi-resolution STFT loss (csrc/stft_loss.hip).  spec_x, spec_y: (B n, 2F) rows [re | im] of one resolution; cnt[b]: the
 * frames of utterance b that count (device int32, clamped to [0, n]); m = sqrt(max(re^2 + im^2, eps)). */
/* frame rows per partial slot of t2amd_stft_loss_fwd_f32 at F bins. */
int t2amd_stft_loss_rows_per_slot(int F);
/* slots[3 s + (0, 1, 2)] = slot s's float64 sums of (m_y - m_x)^2, m_y^2 and |ln m_x - ln m_y| over its rows' frames j < cnt[b];
 * ceil(B n / rows_per_slot) slots, each with one writer. */
int t2amd_stft_loss_fwd_f32(const float* spec_x, long long ldx, const float* spec_y, long long ldy, const int* cnt, int B, int n,
                            int F, float eps, double* slots, long long slot_doubles, void* stream);
/* One launch over R <= 8 resolutions: resolution r owns the slots [slot_off[r], slot_off[r + 1]) (host array of R + 1) and
 * counts[r] = C_r = F_r sum_b cnt[r][b] (host array of R).  With A, Bn, Lm its three sums added in a fixed order in float64:
 * terms[r] = (sc_r, lm_r) = (sqrt(A) / sqrt(Bn), Lm / C_r), sc_r = 0 where A == 0; coef[r] = (sc_weight / (R sqrt(A) sqrt(Bn)),
 * 0 where A == 0; mag_weight / (R C_r)); loss[0] = sum_r (sc_weight sc_r + mag_weight lm_r) / R.  Bn == 0 gives a non-finite loss. */
int t2amd_stft_loss_finish_f64(const double* slots, long long slot_doubles, const long long* slot_off, const double* counts,
                               int R, float sc_weight, float mag_weight, float* loss, float* terms, float* coef, void* stream);
/* d_spec[r] = [d_re (F) | d_im (F) | 0 (Kp - 2F)]: d_m = coef[0] (m_x - m_y) + coef[1] sign(ln m_x - ln m_y) / m_x,
 * d_re = g[0] d_m re / m_x, d_im = g[0] d_m im / m_x where re^2 + im^2 >= eps; exactly 0 below eps and on the frames j >= cnt[b]. */
int t2amd_stft_loss_bwd_f32(const float* spec_x, long long ldx, const float* spec_y, long long ldy, const int* cnt,
                            const float* coef, const float* g, int B, int n, int F, int Kp, float eps, float* d_spec,
                            long long ldd, long long d_floats, void* stream);
/* out[i] = ((parts[i] + parts[stride + i]) + ...) + parts[(R - 1) stride + i], i < total, R <= 8. */
int t2amd_stft_loss_sum_f32(const float* parts, long long stride, long long part_floats, int R, long long total, float* out,
                            void* stream);

/* Sample-rate conversion (csrc/resample.hip).  o = orig / gcd, n = new / gcd; x (B, ldx) rows of T samples, y (B, ldy) rows of
 * Tout = ceil(n T / o); lengths[b]: the samples of utterance b (device int32, clamped to [0, T]; NULL: all T).  No atomics. */
/* The tile of a launch with P phases of S taps, input period I and first-tap + S <= Kd: *npw = outputs per workgroup, *tab_lds =
 * 1 when the phase table is staged in LDS, 0 when it is read from memory.  An error when the table holds more than 2^24 taps or
 * the input window of 256 outputs exceeds 4096 samples. */
int t2amd_resample_plan(int P, int I, int S, int Kd, int* npw, int* tab_lds);
/* y[b][q n + j] = sum_s tab[j][s] xpad[q o + first[j] + s], ascending s, xpad = x[b] with `width` zeros in front and zeros at and
 * beyond lengths[b] whatever the buffer holds; tab (n, S), first (n) with first[j] + S <= 2 width + o.  All Tout columns are
 * written, exact zeros at and beyond ceil(n lengths[b] / o). */
int t2amd_resample_fwd_f32(const float* x, long long ldx, const int* lengths, int B, long long T, float* y, long long ldy,
                           long long Tout, const float* tab, const int* first, int o, int n, int S, int width, void* stream);
/* The adjoint as a gather: d_x[b][q o + r] = sum_s btab[r][s] d_ypad[q n + bfirst[r] + s], ascending s (ascending output index),
 * d_ypad = d_y[b] with `wpad` zeros in front, not read at and beyond ceil(n lengths[b] / o); btab (o, Sb), bfirst (o) with
 * bfirst[r] + Sb <= Kd.  All T columns are written, exact zeros at and beyond lengths[b]. */
int t2amd_resample_bwd_f32(const float* d_y, long long ldy, const int* lengths, int B, long long T, long long Tout, float* d_x,
                           long long ldx, const float* btab, const int* bfirst, int o, int n, int Sb, int wpad, int Kd,
                           void* stream);

/* Mel-cepstral distortion under dynamic time warping (csrc/dtw.hip).  No atomics, one writer per element. */
/* Rows of a band of the DTW wavefront = lanes of its workgroup. */
int t2amd_dtw_width(void);
/* out (B, T, K) contiguous: out[b][t][k] = sum_m basis[k][m] mel[b * ldb + m * ldm + t], ascending m; basis (K, n_mel) contiguous,
 * 1 <= K <= 32, K n_mel <= 8192.  Rows at and beyond lengths[b] (device int32, clamped to [0, T]; NULL: all T) are zeros. */
int t2amd_mel_cepstrum_f32(const float* mel, long long ldb, long long ldm, const int* lengths, int B, int n_mel, int T,
                           const float* basis, int K, float* out, void* stream);
/* Pair p: a + p sa holds n_a rows of K floats, b + p sb holds n_b rows; n_a = na[p], n_b = nb[p] (device int32, NULL: Ta, Tb),
 * 1 to 4096 each.  d(i,j) = sqrt(sum_k (a_ik - b_jk)^2); D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)), D(0,0) = d(0,0);
 * among equal predecessors the diagonal, then (i-1,j), then (i,j-1).  cost[p] = D(n_a-1, n_b-1), steps[p] = the cells of that
 * path.  path (NULL: not wanted): per pair a slab of path_rows x path_cols bytes, byte [i path_cols + j] = the predecessor chosen
 * at (i,j): 0, 1 or 2 in the order above; bytes outside the pair's own n_a x n_b cells are not written. */
int t2amd_dtw_f32(const float* a, long long sa, const float* b, long long sb, const int* na, const int* nb, int B, int Ta, int Tb,
                  int K, float* cost, int* steps, unsigned char* path, int path_rows, int path_cols, void* stream);
/* out (B, L, 2) int32: the path of pair p as (i, j) from (0,0) to (n_a-1, n_b-1), steps[p] entries, then -1.  One lane per pair. */
int t2amd_dtw_backtrack(const unsigned char* path, int path_rows, int path_cols, const int* na, const int* nb, const int* steps,
                        int B, int Ta, int Tb, int* out, int L, void* stream);

/* F0 extraction by YIN (csrc/yin.hip).  No atomics, one writer per element. */
/* The lag range of a geometry: *tau_min = floor(sr / fmax), *tau_max = ceil(sr / fmin).  An error where fmin >= fmax, the frame
 * length L is odd or above 4096, hop < 1, tau_min < 2 or L / 2 + tau_max + 1 > L. */
int t2amd_yin_plan(double sr, int L, int hop, double fmin, double fmax, int* tau_min, int* tau_max);
/* x (B, ldx) rows of T samples; lengths[b]: the samples of utterance b (device int32, clamped to T; NULL: all T).  Utterance b has
 * lengths[b] / hop + 1 frames; frame t is x[t hop - L/2 : t hop + L/2] with zeros outside the utterance.  Per frame:
 * d(tau) = sum_{j < L/2} (f[j] - f[j+tau])^2, d'(tau) = d(tau) tau / (d(1) + .. + d(tau)) (1 where that sum is 0, d'(0) = 1); the lag
 * is the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, d'(tau) < d'(tau-1) and d'(tau) <= d'(tau+1) (voiced), else the
 * first argmin of d' over the range (unvoiced); f0 = sr / (tau + shift) with the parabolic shift clipped to half a lag.
 * f0, voiced (bytes 0 / 1), aperiodicity = d'(tau): (B, frames) contiguous, frames = T / hop + 1, zeros at and beyond an
 * utterance's count.  dprime (NULL: not wanted): (B, frames, tau_max + 2) contiguous, d'(0 .. tau_max + 1), zeros likewise. */
int t2amd_yin_f32(const float* x, long long ldx, const int* lengths, int B, long long T, int frames, int L, int hop, int tau_min,
                  int tau_max, float sr, float threshold, float* f0, unsigned char* voiced, float* aperiodicity, float* dprime,
                  void* stream);

/* Forced alignment: the best monotonic path through a (frames, tokens) score matrix (csrc/align.hip).  No
 * atomics, one writer per element. */
/* *width = lanes of the workgroup, *max_frames = 4096, *max_tokens = 1024. */
int t2amd_align_limits(int* width, int* max_frames, int* max_tokens);
/* *bytes = the workspace of a launch over B utterances of at most T_max frames and N_max tokens: one byte per cell at a row of
 * N_max rounded up to 4, then two 64-bit counts of the 100 MHz clock per utterance (the recurrence, the backtrack). */
int t2amd_align_workspace(int B, int T_max, int N_max, long long* bytes);
/* scores[b * sb + t * st + n], t < t_len[b] <= T_max <= 4096, n < n_len[b] <= N_max <= 1024 (device int32; the host has refused
 * every utterance without 1 <= n_len <= t_len).  Q(0,0) = l(0,0), Q(0,n>0) = -inf, Q(t,n) = l(t,n) + max(Q(t-1,n), Q(t-1,n-1)),
 * staying wins ties; the path runs from (0,0) to (t_len-1, n_len-1) in steps of 0 or 1 tokens a frame.  durations (B, N_max)
 * int32: frames on each token, zeros at and beyond n_len[b]; score (B,) = Q(t_len-1, n_len-1); path (NULL: not wanted)
 * (B, T_max) int32: the token of every frame, -1 at and beyond t_len[b].  ws: ws_bytes >= t2amd_align_workspace's, 8-byte
 * aligned; of utterance b's slab only rows 1 .. t_len-1 and columns below n_len rounded up to 4 are written. */
int t2amd_monotonic_align_f32(const float* scores, long long sb, long long st, const int* t_len, const int* n_len, int B, int T_max,
                              int N_max, int* durations, float* score, int* path, unsigned char* ws, long long ws_bytes,
                              void* stream);

/* Forward-sum alignment likelihood and its gradient over the same paths (csrc/forward_sum.hip):
 * a(0,0) = l(0,0), a(0,n>0) = -inf, a(t,n) = l(t,n) + logaddexp(a(t-1,n), a(t-1,n-1)), log Z = a(t_len-1, n_len-1); b the same
 * from the other end; gamma(t,n) = exp(a + b - log Z) = d log Z / d l(t,n).  logaddexp(-inf, -inf) = -inf; an utterance without
 * a possible path has log Z = -inf and zero gamma.  Rows are kept relative to float64 offsets renewed every 16 rows.  Lengths
 * and limits are those of t2amd_monotonic_align_f32.  No atomics, one writer per element. */
/* *bytes = the workspace of a launch over B utterances: with `keep`, the alpha rows (float32, a row of N_max rounded up to 4)
 * and one float64 offset per row; always, at its tail, two 64-bit counts of the 100 MHz clock per utterance (the alpha
 * launch, the beta launch). */
int t2amd_forward_sum_workspace(int B, int T_max, int N_max, int keep, long long* bytes);
/* log_z (B,) float32.  keep != 0: the alpha rows and their offsets go to ws for t2amd_forward_sum_bwd_f32 (of utterance b's
 * slab only rows below t_len and columns below n_len, rounded up to 4 where N_max > 256, are written).  ws: ws_bytes >=
 * t2amd_forward_sum_workspace's for the same `keep`, 16-byte aligned. */
int t2amd_forward_sum_f32(const float* scores, long long sb, long long st, const int* t_len, const int* n_len, int B, int T_max,
                          int N_max, float* log_z, int keep, unsigned char* ws, long long ws_bytes, void* stream);
/* grad[b * gb + t * gt + n] = scale[b] gamma(t,n) (scale NULL: 1) for t < T_max, n < N_max, exact zeros at t >= t_len or
 * n >= n_len; soft (NULL: not wanted) (B, N_max) = sum_t gamma(t,n), zeros at and beyond n_len.  scores, lengths, log_z and ws
 * are those of a t2amd_forward_sum_f32 call with keep != 0. */
int t2amd_forward_sum_bwd_f32(const float* scores, long long sb, long long st, const int* t_len, const int* n_len, int B, int T_max,
                              int N_max, const float* log_z, const float* scale, float* grad, long long gb, long long gt,
                              float* soft, unsigned char* ws, long long ws_bytes, void* stream);

/* Learned-aligner scores and their gradient (csrc/aligner.hip, csrc/aligner_rows.hip): per utterance b
 * with t_len[b] frames and n_len[b] tokens (device int32, 1 <= t_len <= T_max <= 4096, 1 <= n_len <= N_max <= 1024), queries
 * q (B, T_max, C) and keys k (B, N_max, C) contiguous float32, 1 <= C <= 512, temperature tau > 0:
 *   z(t,n) = tau (2 q_t . k_n - |k_n|^2), lse(t) = log sum_{n < n_len} exp z(t,n), s(t,n) = z(t,n) - lse(t) + logp(t,n),
 * -inf at t >= t_len or n >= n_len.  No atomics, one writer per element, sums in a fixed order. */
/* *bytes = a workspace: which 0 the forward's (the key slab, a row of C rounded up to 32, and the key norms), 1 the same with
 * the row logsumexp kept for the backward, 2 the backward's own (dz at a row of N_max rounded up to 32, both operands
 * transposed, the column sums of dz). */
int t2amd_aligner_workspace(int B, int T_max, int N_max, int C, int which, long long* bytes);
/* Kp (B, N_max, C rounded up to 32) = k with zeros beyond C and in rows at and beyond n_len; kn (B, N_max) = |k_n|^2. */
int t2amd_aligner_pack_keys_f32(const float* k, const int* n_len, int B, int N_max, int C, float* Kp, float* kn, void* stream);
/* out (B, C, R_max rounded up to 32): out[b][c][r] = x[b][r][c] for r < lens[b], zeros beyond; x (B, R_max, C). */
int t2amd_aligner_transpose_f32(const float* x, const int* lens, int B, int R_max, int C, float* out, void* stream);
/* The row pass of the forward, in place: scores[b * sb + t * st + n] holds z inside every utterance and leaves holding s, -inf
 * in the padding; logp (NULL: none) at (pb, pt); lse (NULL: not kept) (B, T_max), written below t_len. */
int t2amd_aligner_rows_fwd_f32(float* scores, long long sb, long long st, const float* logp, long long pb, long long pt,
                               const int* t_len, const int* n_len, int B, int T_max, int N_max, float* lse, void* stream);
/* The row pass of the backward: dz (B, T_max, N_max rounded up to 32) holds z inside every utterance and leaves holding
 * dz = g - exp(z - lse) sum_n g, zeros elsewhere; colsum (B, N_max) = sum_t dz (float64 sums, rounded once; zeros at and beyond
 * n_len); dlogp (NULL: not wanted) at (db, dt) = g inside an utterance, zeros outside.  g at (gb, gt). */
int t2amd_aligner_rows_bwd_f32(const float* g, long long gb, long long gt, const int* t_len, const int* n_len, int B, int T_max,
                               int N_max, const float* lse, float* dz, float* colsum, float* dlogp, long long db, long long dt,
                               void* stream);
/* scores (at sb, st) = s.  keep != 0 leaves in ws what t2amd_aligner_scores_bwd_f32 reads.  ws: ws_bytes >=
 * t2amd_aligner_workspace's for which = (keep != 0), 16-byte aligned.  q and k need no alignment: the query rows are
 * fetched four at a time where C is a multiple of 4 and q starts on 16 bytes, one at a time otherwise, with the same bits. */
int t2amd_aligner_scores_f32(const float* q, const float* k, const int* t_len, const int* n_len, int B, int T_max, int N_max, int C,
                             float tau, const float* logp, long long pb, long long pt, float* scores, long long sb, long long st,
                             int keep, unsigned char* ws, long long ws_bytes, void* stream);
/* Given g = dL/ds at (gb, gt) (its padding is ignored): dq (B, T_max, C) and dk (B, N_max, C) contiguous, exact zeros in the
 * padding; dlogp (NULL: not wanted) at (db, dt).  `kept` is the workspace of a t2amd_aligner_scores_f32 call with keep != 0 on the
 * same operands, ws the backward's own (which = 2). */
int t2amd_aligner_scores_bwd_f32(const float* q, const float* k, const int* t_len, const int* n_len, int B, int T_max, int N_max,
                                 int C, float tau, const float* g, long long gb, long long gt, float* dq, float* dk, float* dlogp,
                                 long long db, long long dt, const unsigned char* kept, long long kept_bytes, unsigned char* ws,
                                 long long ws_bytes, void* stream);
/* One product of t2amd_aligner_scores_bwd_f32 alone, on its operands and workspaces (for timing a product by itself; the
 * backward calls it three times): which 1 z into the dz slab of ws, 2 dQ from the dz and KT slabs, 3 dK from the dz and QT slabs
 * and the column sums.  dq may be NULL unless which is 2, dk unless it is 3. */
int t2amd_aligner_product_f32(int which, const float* q, const float* k, const int* t_len, const int* n_len, int B, int T_max,
                              int N_max, int C, float tau, float* dq, float* dk, const unsigned char* kept, long long kept_bytes,
                              unsigned char* ws, long long ws_bytes, void* stream);
/* out (B, T_max, N_max) contiguous: the beta-binomial log prior of frame t over the tokens, a = scaling (t + 1),
 * b = scaling (t_len - t), m = n_len - 1: lgamma(m+1) - lgamma(n+1) - lgamma(m-n+1) + lbeta(n + a, m - n + b) - lbeta(a, b) in
 * float64, rounded once; -inf in the padding. */
int t2amd_beta_binomial_log_prior_f32(const int* t_len, const int* n_len, int B, int T_max, int N_max, double scaling, float* out,
                                      void* stream);

/* The length regulator (csrc/regulate.hip): per utterance b with n_len[b] tokens (device int32, clamped
 * into [0, N_max]; NULL: N_max) and durations d(n) >= 0, e(n) = d(0) + .. + d(n) (64-bit, a term counts as at most 2^31 - 1),
 * S = e(n_len - 1), T_b = min(S, T); path(t) = the smallest n < n_len with e(n) > t for t < T_b and -1 for T_b <= t < T.
 * 1 <= B <= 65535, 1 <= N_max <= 1024, T <= 65536, 1 <= C <= 512.  No atomics, one writer per element, sums in a fixed order. */
/* *max_channels = 512, *max_tokens = 1024, *max_frames = 65536. */
int t2amd_regulate_limits(int* max_channels, int* max_tokens, int* max_frames);
/* durations[b * db + n], int32 (duration_bytes 4) or int64 (8); those at and beyond n_len[b] are not read.  t_lengths (B,) = T_b;
 * path (NULL: not wanted) (B, T) int32; ends (NULL: not wanted) (B, N_max) int32 = min(e(n), T), T_b at and beyond n_len;
 * totals (NULL: not wanted) (B,) int64 = S.  T may be 0.  An utterance with a negative duration below n_len is marked:
 * t_lengths = -1, totals = -1, ends 0, path -1. */
int t2amd_durations_to_path_i32(const void* durations, int duration_bytes, long long db, const int* n_len, int B, int N_max, int T,
                                int* path, int* t_lengths, int* ends, long long* totals, void* stream);
/* y (B, T, C) contiguous: y(t, :) = x(path(t), :), +0 where path(t) = -1; x[b * xb + n * xn + c].  Rows move 16 bytes at a
 * time where C is a multiple of 4, x and y start on 16 bytes and the strides are multiples of 4, one float at a time
 * otherwise, with the same bits.  1 <= T. */
int t2amd_length_regulate_f32(const float* x, long long xb, long long xn, const int* path, int B, int N_max, int T, int C, float* y,
                              void* stream);
/* dx (B, N_max, C) contiguous: dx(n, :) = the sum of dy(t, :) over t = ends(n-1) .. ends(n) - 1 ascending (ends(-1) = 0), plain
 * float32 adds from the first term, +0 for an empty range; dy[b * gb + t * gt + c]; ends as t2amd_durations_to_path_i32 wrote. */
int t2amd_length_regulate_bwd_f32(const float* dy, long long gb, long long gt, const int* ends, int B, int N_max, int T, int C,
                                  float* dx, void* stream);
/* Over the same ranges: num(n, c) = fmaf(w(t), v(t, c), num) from +0, den(n) = den + w(t) from +0 (w NULL: 1), m = num / den where
 * den > 0 and +0 elsewhere.  v[b * vb + t * vt + c], w[b * wb + t]; m and num (NULL: not wanted) (B, N_max, C), den (B, N_max). */
int t2amd_token_average_f32(const float* v, long long vb, long long vt, const float* w, long long wb, const int* ends, int B,
                            int N_max, int T, int C, float* m, float* den, float* num, void* stream);
/* dv (B, T, C) contiguous: dv(t, c) = w(t) * (g(path(t), c) / den(path(t))), +0 where path(t) = -1 or den = 0; g (B, N_max, C)
 * and den (B, N_max) contiguous. */
int t2amd_token_average_bwd_f32(const float* g, const float* den, const float* w, long long wb, const int* path, int B, int N_max,
                                int T, int C, float* dv, void* stream);

/* Masked multi-head self-attention (csrc/self_attn.hip, csrc/self_attn_rows.hip): per utterance b with
 * T_b = lengths[b] frames (device int32, clamped into [0, T]; NULL: T) and per head h, s(t, j) = scale sum_d q(t, d) k(j, d),
 * p = softmax over j < T_b, o(t, :) = sum_j p(t, j) v(j, :) for t < T_b and +0 from there on; lse(t) = log sum_j exp s(t, j).
 * Element (b, t, h, d) of q, k, v and g lies at x[b * xb + t * xt + h * xh + d]: strides that are multiples of 4 floats, bases
 * aligned to 16 bytes; what lies at and beyond T_b is never read.  o, dq, dk, dv are contiguous (B, T, H, D), lse (B, H, T).
 * D in {32, 64, 96, 128}, 1 <= H <= 16, T <= 4096, B H <= 65535.  Exact f32, no atomics, one writer per element, every sum in a
 * fixed ascending order.  Error texts begin with "self_attn:". */
/* *max_frames = 4096, *max_heads = 16, *min_width = 32, *max_width = 128, *max_batch_heads = 65535. */
int t2amd_self_attn_limits(int* max_frames, int* max_heads, int* min_width, int* max_width, int* max_batch_heads);
/* which 0: the forward's workspace (none: 0 bytes); 1: the bytes of the lse the forward writes for a backward; 2: the
 * backward's workspace (delta, (B, H, T)). */
int t2amd_self_attn_workspace(int B, int T, int H, int D, int which, long long* bytes);
/* lse NULL: not kept. */
int t2amd_self_attn_f32(const float* q, long long qb, long long qt, long long qh, const float* k, long long kb, long long kt,
                        long long kh, const float* v, long long vb, long long vt, long long vh, const int* lengths, int B, int T,
                        int H, int D, float scale, float* o, float* lse, void* stream);
/* delta (B, H, T): delta(t) = sum_d g(t, d) o(t, d) as an fmaf chain per lane over d = lane, lane + 64 and a xor butterfly; +0
 * at and beyond T_b.  The first launch of the backward, callable alone. */
int t2amd_self_attn_delta_f32(const float* g, long long gb, long long gt, long long gh, const float* o, const int* lengths, int B,
                              int T, int H, int D, float* delta, void* stream);
/* dq, dk, dv from g = dL/do; o and lse are what t2amd_self_attn_f32 wrote on the same operands; ws holds at least
 * t2amd_self_attn_workspace(.., 2) bytes.  All three gradients are +0 at and beyond T_b. */
int t2amd_self_attn_bwd_f32(const float* q, long long qb, long long qt, long long qh, const float* k, long long kb, long long kt,
                            long long kh, const float* v, long long vb, long long vt, long long vh, const float* o, const float* lse,
                            const float* g, long long gb, long long gt, long long gh, const int* lengths, int B, int T, int H, int D,
                            float scale, float* dq, float* dk, float* dv, unsigned char* ws, long long ws_bytes, void* stream);

/* The feed-forward Transformer block's convolutional feed-forward and add + LayerNorm (csrc/fft_block.hip,
 * csrc/fft_block_rows.hip) over a ragged batch: utterance b has T_b = lengths[b] frames (device int32,
 * clamped into [0, T]; NULL: T).  Every tensor is float32, channel-last and contiguous (B, T, C), but a convolution's input x,
 * whose element (b, t, i) lies at x[b * xb + t * xt + i] (strides that are multiples of 4 floats, a base aligned to 16 bytes).
 * Each utterance is convolved as if it were alone: frames outside [0, T_b) are absent.  Rows at and beyond T_b are never read and
 * every output is +0 there.  Channels of a convolution are multiples of 32, at most 4096; k is odd, at most 9; T <= 4096;
 * B <= 65535; LayerNorm channels are multiples of 4 from 32 to 4096.  Exact f32, no atomics, one writer per element, every sum in
 * a fixed order.  Error texts begin with "fft_block:". */
/* *max_frames = 4096, *max_channels = 4096, *max_taps = 9, *min_norm_channels = 32, *max_batch = 65535. */
int t2amd_fft_block_limits(int* max_frames, int* max_channels, int* max_taps, int* min_norm_channels, int* max_batch);
/* which 0: t2amd_ffb_conv_f32 (none: 0 bytes); 1: t2amd_ffb_conv_dw_f32 (the transposed gradient slab and the slices' partial
 * sums); 2: t2amd_ffb_colsum_f32 over Cout channels (the partial sums; Cin and k are not read). */
int t2amd_fft_block_workspace(int B, int T, int Cin, int Cout, int k, int which, long long* bytes);
/* y(b, t, o) = act(bias(o) + sum_{j, i} image[o][j Cin + i] x(b, t + j - k/2, i)) for t < T_b, an fmaf chain over j then i
 * ascending from +0, then the bias.  image is [Cout][k Cin]; bias NULL: none; relu != 0: max(., 0); mask (B, T, Cout) non-NULL:
 * the value is kept only where mask > 0.  The input gradient is the same call on the image of the flipped, transposed weights. */
int t2amd_ffb_conv_f32(const float* x, long long xb, long long xt, const float* image, const float* bias, const float* mask,
                       const int* lengths, int B, int T, int Cin, int Cout, int k, int relu, float* y, void* stream);
/* dw (Cout, Cin, k) = sum over b, then t ascending of g(b, t, o) x(b, t + j - k/2, i): the reduction index b Tp + t (Tp = T
 * rounded up to 32) is cut into slices that depend on B and T alone, each an ascending fmaf chain, added in ascending order. */
int t2amd_ffb_conv_dw_f32(const float* g, const float* x, long long xb, long long xt, const int* lengths, int B, int T, int Cin,
                          int Cout, int k, float* dw, unsigned char* ws, long long ws_bytes, void* stream);
/* The two row passes of t2amd_ffb_conv_dw_f32, callable alone: the slab of g (B, T, C) transposed per slice, and the slice sum. */
int t2amd_ffb_transpose_f32(const float* g, const int* lengths, int B, int T, int C, float* out, long long out_bytes, void* stream);
int t2amd_ffb_dw_finish_f32(const float* part, int slices, int Cin, int Cout, int k, float* dw, void* stream);
/* y = LayerNorm(x + residual) weight + bias per row t < T_b (two-pass variance).  residual NULL: none.  weight and bias NULL: y is
 * x + residual itself ("add and mask"; mean and rstd must then be NULL).  z (B, T, C), mean and rstd (B, T) non-NULL: kept for
 * the backward (z = x + residual). */
int t2amd_ffb_add_ln_f32(const float* x, const float* residual, const float* weight, const float* bias, const int* lengths, int B,
                         int T, int C, float eps, float* y, float* z, float* mean, float* rstd, void* stream);
/* dz = the LayerNorm input gradient of g, from the kept z, mean and rstd. */
int t2amd_ffb_add_ln_bwd_f32(const float* g, const float* z, const float* mean, const float* rstd, const float* weight,
                             const int* lengths, int B, int T, int C, float* dz, void* stream);
/* dbias(c) = sum of g(b, t, c), dweight(c) = sum of g (z - mean) rstd over the real rows: partial sums over runs of the flattened
 * (b, t), then their ascending sum.  z NULL: dbias alone (a convolution's). */
int t2amd_ffb_colsum_f32(const float* g, const float* z, const float* mean, const float* rstd, const int* lengths, int B, int T,
                         int C, float* dbias, float* dweight, unsigned char* ws, long long ws_bytes, void* stream);
/* out = g where y > 0 and +0 elsewhere: the gradient below a ReLU. */
int t2amd_ffb_relu_mask_f32(const float* g, const float* y, const int* lengths, int B, int T, int C, float* out, void* stream);

/* The thin ends of a temporal predictor (csrc/predictor_rows.hip), which the ragged convolution above
 * cannot express: the projection of C channels onto P values per row and the embedding of P scalar tracks into C channels with k
 * taps, over a ragged batch as above (lengths: device int32, clamped into [0, T]; NULL: T).  Float32, contiguous, channel-last:
 * h, base, y of the embedding, g of the embedding (B, T, C) on 16 bytes; the tracks v and the projection's y and g (B, T, P).
 * 1 <= P <= 4; k odd, at most 9; C a multiple of 4 from 32 to 4096; T <= 4096; B <= 65535.  Rows at and beyond T_b are never read
 * and every output is +0 there.  Row kernels: one wave per row, no atomics, one writer per element, every sum in a fixed order.
 * Error texts begin with "predictor:". */
/* *max_frames = 4096, *max_channels = 4096, *max_taps = 9, *max_tracks = 4, *max_batch = 65535. */
int t2amd_predictor_limits(int* max_frames, int* max_channels, int* max_taps, int* max_tracks, int* max_batch);
/* which 0: the forwards and the input gradients (none: 0 bytes); 1: t2amd_pred_project_sums_f32 (k is checked, not used); 2:
 * t2amd_pred_embed_sums_f32. */
int t2amd_predictor_workspace(int B, int T, int C, int P, int k, int which, long long* bytes);
/* y(b, t, p) = bias(p) + sum_c w(p, c) h(b, t, c) for t < T_b: lane l of 64 chains fmaf over the components of the float4 chunks
 * l, l + 64, .. from +0, the xor butterfly 32 .. 1, then the bias.  w is [P][C]; bias [P] or NULL. */
int t2amd_pred_project_f32(const float* h, const float* w, const float* bias, const int* lengths, int B, int T, int C, int P, float* y,
                           void* stream);
/* dh(b, t, c) = sum_p g(b, t, p) w(p, c), an fmaf chain over p ascending from +0. */
int t2amd_pred_project_bwd_f32(const float* g, const float* w, const int* lengths, int B, int T, int C, int P, float* dh, void* stream);
/* dw(p, c) = sum of g(b, t, p) h(b, t, c) (fmaf) and db(p) = sum of g(b, t, p) (adds) over the real rows: partial sums over runs of
 * the flattened (b, t) ascending, then the partials ascending from +0.  dw or db may be NULL, not both. */
int t2amd_pred_project_sums_f32(const float* g, const float* h, const int* lengths, int B, int T, int C, int P, float* dw, float* db,
                                unsigned char* ws, long long ws_bytes, void* stream);
/* y(b, t, c) = base(b, t, c) + (bias(c) + sum_{p, j} image[p k + j][c] v(b, t + j - k/2, p)) for t < T_b over the frames inside
 * [0, T_b) only: an fmaf chain over p then j ascending from +0, then the bias, then the base.  image is [P k][C] with
 * image[p k + j][c] = w(c, p, j); bias [C] or NULL; base (B, T, C) or NULL. */
int t2amd_pred_embed_f32(const float* v, const float* image, const float* bias, const float* base, const int* lengths, int B, int T,
                         int C, int P, int k, float* y, void* stream);
/* dbase (B, T, C) = g masked to the real rows; dv(b, t, p) = sum over j ascending of u(b, t - j + k/2, p, j) over the rows inside
 * the utterance, u(b, t, p, j) = sum_c image[p k + j][c] g(b, t, c) in the order of t2amd_pred_project_f32.  dbase or dv may be
 * NULL, not both; image may be NULL without dv. */
int t2amd_pred_embed_bwd_f32(const float* g, const float* image, const int* lengths, int B, int T, int C, int P, int k, float* dbase,
                             float* dv, void* stream);
/* dw (C, P, k) = sum of g(b, t, c) v(b, t + j - k/2, p) (fmaf) and db(c) = sum of g(b, t, c) (adds) over the real rows, by the
 * partial sums of t2amd_pred_project_sums_f32.  dw or db may be NULL, not both. */
int t2amd_pred_embed_sums_f32(const float* g, const float* v, const int* lengths, int B, int T, int C, int P, int k, float* dw,
                              float* db, unsigned char* ws, long long ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Griffin-Lim vocoder (csrc/vocoder.hip): element passes around the two GEMMs of one
 * Griffin-Lim iteration (reference audio_processing.py:59-76, stft.py:77-141).  The contractions are
 * t2amd_gemm_f32 calls (precision 0 exact f32 or 1 split-bf16):
 *   frames[r][L] = rec[r][2Fp] . IB[L][2Fp]^T     IB = windowed pinv(scale * fourier_basis), columns interleaved
 *   spec[r][2F]  = padded-as-[R][L] (lda = hop) . FB[2F][L]^T      FB rows interleaved (re, im)
 * Complex rows are interleaved: [2f] real, [2f+1] imaginary; columns 2F .. 2Fp of rec are zero.
 * Packed frame space: utterance b (n_b frames) owns rows [row0_b, row0_b + n_b + ceil(L/hop) - 1) and its
 * reflect-padded signal starts at sample row0_b * hop of one packed buffer.  `plan` (int32, device) is
 *   [row0_0 .. row0_{B-1}, R | n_0 .. n_{B-1} | utterance of row 0 .. R-1]   (2B + 1 + R entries);
 * `n_host` is the same n_b on the host, checked by every entry point: (n_b - 1) * hop > L / 2 (reflect padding)
 * and sum(n_b + ceil(L/hop) - 1) == R.  All launches are 1-D grid-stride: no 65,535-row limit.
 * ------------------------------------------------------------------------------------ */
/* sum(n_b + ceil(L/hop) - 1), or -1 for bad arguments (host only) */
long long t2amd_gl_packed_rows(const int* n_host, int B, int L, int hop);
/* Overlap-add of the inverse transform: every output sample sums the frames that cover it in ascending frame order, is
 * divided by the float32 window sum-square (rebuilt from the float64 squared-window table wsq[L]) where that is
 * > tiny(float32), and is multiplied by `scale` (= L / hop).  mode 0: out = the reflect-padded packed signal of the next
 * forward transform (out_len >= (R - 1) * hop + L samples; gaps and tail zero).  mode 1: out[b][s] (row stride ldo,
 * s < out_len) = the trimmed signal of utterance b for s < (n_b - 1) * hop, 0 beyond. */
int t2amd_gl_overlap_add_f32(const float* frames, long long ldf, const double* wsq, const int* plan, const int* n_host,
                             int B, long long R, int L, int hop, float scale, float* out, long long ldo, long long out_len,
                             int mode, void* stream);
/* rec[r][2f, 2f+1] = S[r][f] * (re, im) / |re + i im| for valid rows and f < F ((S, 0) when |z| = 0); zeros in gap rows
 * and pad columns.  spec, rec: 8-byte aligned, even row strides. */
int t2amd_gl_project_f32(const float* spec, long long lds, const float* S, long long ldS, const int* plan,
                         const int* n_host, int B, long long R, int L, int hop, int F, int Fp, float* rec, long long ldr,
                         void* stream);
/* rec[r][2f, 2f+1] = m (cos p, sin p) with m = mag[b][f][j], p = phase[b][f][j] ((B, F, ldn) contiguous; phase NULL: 0)
 * for row r = row0_b + j; S[r][f] = m.  mag NULL: m is read from S instead (S is not written). */
int t2amd_gl_rect_f32(const float* mag, const float* phase, long long ldn, const int* plan, const int* n_host, int B,
                      long long R, int L, int hop, int F, int Fp, float* S, long long ldS, float* rec, long long ldr,
                      void* stream);
/* spec rows (B*n, interleaved) -> mag[b][f][j] = sqrt(re^2 + im^2), phase[b][f][j] = atan2(im, re), (B, F, n) contiguous;
 * either output may be NULL. */
int t2amd_stft_polar_f32(const float* spec, long long lds, int B, int n, int F, float* mag, float* phase, void* stream);
/* out[(b*n + j)*ld + m] = exp(mel[b][m][j]) for m < n_mel and j < lengths[b] (device; NULL: every j), 0 otherwise:
 * the inverse of t2amd_mel_log_compress_f32.  n_host: the lengths on the host (for the checks) when lengths is set. */
int t2amd_mel_decompress_f32(const float* mel, int B, int n_mel, int n, const int* lengths, const int* n_host, float* out,
                             long long ld, void* stream);

/* ------------------------------------------------------------------------------------
 * WaveGlow inference (csrc/waveglow.hip, csrc/waveglow_layer.hip; tacotron2_amd/waveglow.py).  NVIDIA's glow.py is not
 * part of the reference checkout: the arithmetic these passes follow is restated in tests/waveglow_ref.py.
 * Packed row space: utterance b's rows (n_group samples each) sit between zero halos of `halo` rows, [halo | R_0 | halo |
 * ... | R_{B-1} | halo]; rowb[p] is the utterance of packed row p (-1 in a halo), rowr[p] its row in the utterance.
 * ------------------------------------------------------------------------------------ */
/* One WN layer product over M rows of the image X (row stride ldx, X at the first computed row; the image carries a zero
 * halo of at least dil rows on both sides).  W [N][taps * Cin], K tap-major: column tap * Cin + c reads
 * X[(m + (tap - (taps-1)/2) * dil) * ldx + c].  precision 0 exact f32, 1 split-bf16 x3, 2 bf16.
 * mode 0 (gated, N = 2C, C a multiple of 64): W rows / bias packed so that block 64q .. 64q+31 holds tanh channels
 *   32q .. 32q+31 and 64q+32 .. 64q+63 their sigmoid partners;  acts[m][c] = tanh(. + cnd[m][c]) * sigmoid(. + cnd[m][C+c])
 *   with cnd in the original column order.
 * mode 1 (residual / skip, taps 1): column n < nres: h[m][n] += . (rows with rowb[m] >= 0 only); n >= nres:
 *   skip[m][n - nres] = . (skip_store) or += . */
int t2amd_wg_layer_f32(const float* X, long long ldx, const float* W, const float* bias, int M, int N, int Cin, int taps,
                       int dil, int mode, const float* cnd, long long ldcnd, float* acts, long long ldacts, float* h,
                       long long ldh, int nres, float* skip, long long ldskip, int skip_store, const int* rowb,
                       int precision, void* stream);
/* Flow tail over P packed rows (rows with rowb >= 0), f32: e = end_b + end_w[n_in][C] . skip[p];
 * x1 = (x1 - e[:n_in/2]) / exp(e[n_in/2:]) on x = audio[p][0:n_in]; y = winv[n_in][n_in] . x;
 * a = [sigma * z[b*zb + k*zc + r] for k < n_new ; y] (z NULL: a = y; end_w NULL: a = the noise alone, the first call);
 * out[b*ldout + n_group*r + g] = a[g] when out is set (the waveform, after flow 0), else audio[p] = a;
 * h[p][c] = start_b[c] + start_w[c][0:n_out/2] . a when start_w is set.  C <= 512, even n_group <= 16. */
int t2amd_wg_tail_f32(const float* skip, long long ldskip, int C, const float* end_w, const float* end_b, int n_in,
                      const float* winv, float* audio, long long ldaudio, const float* z, long long zb, long long zc,
                      int n_new, float sigma, const float* start_w, const float* start_b, float* h, long long ldh,
                      float* out, long long ldout, const int* rowb, const int* rowr, long long P, int n_group,
                      void* stream);
/* Denoiser (reference denoiser.py): mag[b][f][t] = max(mag - bias[f] * strength, 0) in place, mag (B, F, n) contiguous. */
int t2amd_wg_denoise_f32(float* mag, const float* bias, int B, int F, long long n, float strength, void* stream);

/* ------------------------------------------------------------------------------------
 * WaveGlow forward direction (csrc/waveglow_fwd.hip; WaveGlow.forward / WaveGlow.nll / WaveGlowLoss): audio to latents and
 * the terms of the negative log-likelihood.  The products are the ones inference runs; the packed row space is the same.
 * ------------------------------------------------------------------------------------ */
/* Flow head over P packed rows (rows with 0 <= rowb < B and rowr < R; b = rowb[p], r = rowr[p]), f32.  It closes one flow
 * and opens the next:
 *   x = audio[p][0:n_in];  e = end_b + end_w[n_in][C] . skip[p];  x1 = exp(e[n_in/2:]) * x1 + e[:n_in/2];
 *   log_s[b*lsb + j*lsc + r] = e[n_in/2 + j]   (end_w NULL, the first call: x[g] = wave[b*ldwave + n_group*r + g], all
 *   n_group channels, and no flow to close; exactly one of end_w / wave is set);
 *   z[b*zb + (z_off + k)*zc + r] = x[k] for k < n_emit (an early output; on the last call every channel that is left);
 *   a = mix_w[n_out][n_out] . x[n_emit:], n_out = n_in - n_emit;  audio[p][0:n_out] = a;
 *   h[p][c] = start_b[c] + start_w[c][0:n_out/2] . a   (mix_w NULL: the last call, n_emit == n_in, nothing to open).
 * R bounds the rows of one utterance (lsc, zc >= R).  C <= 512, even n_group <= 16. */
int t2amd_wg_head_f32(const float* skip, long long ldskip, int C, const float* end_w, const float* end_b, int n_in,
                      float* log_s, long long lsb, long long lsc, const float* wave, long long ldwave, float* audio,
                      long long ldaudio, float* z, long long zb, long long zc, int z_off, int n_emit, const float* mix_w,
                      const float* start_w, const float* start_b, float* h, long long ldh, const int* rowb,
                      const int* rowr, long long P, int n_group, int B, long long R, void* stream);
/* out[b][0] = sum over c < nz, r < len[b] of z[b*zb + c*zc + r]^2 and out[b][1] = the same sum of ls[b*lb + c*lc + r]
 * over c < nls (ls NULL with nls 0: 0), in double and in a fixed order (two launches, no atomics): an utterance's sums do
 * not depend on the batch it sits in.  len (device) is clamped to [0, R]; partial holds B * nchunk * 2 doubles with
 * nchunk = ceil(R / t2amd_wg_nll_chunk()). */
int t2amd_wg_nll_chunk(void);
int t2amd_wg_nll_f32(const float* z, long long zb, long long zc, int nz, const float* ls, long long lb, long long lc, int nls,
                     const int* len, int B, long long R, double* partial, long long nchunk, double* out, void* stream);

/* ------------------------------------------------------------------------------------
 * WaveGlow backward pass (csrc/waveglow_bwd.hip and the training entries of csrc/waveglow_fwd.hip / waveglow_layer.hip;
 * WaveGlow.training_loss).  loss = (sum z^2 / (2 sigma^2) - sum log_s - sum log det W) / numel; c1 = 1 / (sigma^2 numel),
 * c2 = -1 / numel.  No atomics anywhere: two runs give identical bits.
 * ------------------------------------------------------------------------------------ */
/* t2amd_wg_layer_f32 with the training forward's extra outputs and the data-gradient mode:
 * mode 0, gate != NULL: gate[m][0:C] = the tanh values, gate[m][C:2C] = the sigmoid values of acts (channel order);
 * mode 1, h_out != NULL: h_out[m][n] = h[m][n] + . instead of h[m][n] += . (h itself is left as the layer read it);
 * mode 2 (N = C, taps 3, Cin = 2C, X = the image of d_pre, W [C][3 * 2C] the transposed in-layer weights with the taps
 *   mirrored, bias unused): h[m][n] += . (or = . when skip_store) on rows with rowb[m] >= 0. */
int t2amd_wg_layer_train_f32(const float* X, long long ldx, const float* W, const float* bias, int M, int N, int Cin, int taps,
                             int dil, int mode, const float* cnd, long long ldcnd, float* acts, long long ldacts, float* h,
                             long long ldh, int nres, float* skip, long long ldskip, int skip_store, const int* rowb,
                             float* gate, long long ldgate, float* h_out, long long ldhout, int precision, void* stream);
/* t2amd_wg_head_f32 that also keeps, per real row, sv[p][0:n_cur] = x (after the coupling, before the early output and the
 * mix) and sv[p][n_group:n_group + n_out] = a (after the mix); sv NULL: t2amd_wg_head_f32 itself.  ldsv >= 2 n_group. */
int t2amd_wg_head_save_f32(const float* skip, long long ldskip, int C, const float* end_w, const float* end_b, int n_in,
                           float* log_s, long long lsb, long long lsc, const float* wave, long long ldwave, float* audio,
                           long long ldaudio, float* z, long long zb, long long zc, int z_off, int n_emit,
                           const float* mix_w, const float* start_w, const float* start_b, float* h, long long ldh,
                           const int* rowb, const int* rowr, long long P, int n_group, int B, long long R, float* sv,
                           long long ldsv, void* stream);
/* Backward of one flow head call over P packed rows (t2amd_wg_head_bwd_rows() rows per workgroup).  With x_sv / a_sv the
 * rows that call kept, a_in the a rows of the call before it (the coupling's input), dh0 the gradient of the opened flow's
 * layer-0 input and dA the gradient of the audio rows (in: of the opened flow's, out: of the closed flow's):
 *   da = dA[p][0:n_out] + [start_w^T . dh0[p] | 0];  dx[n_emit:] = mix_w^T . da;  dx[k] = c1 x[k] for k < n_emit;
 *   de = [dx1, dx1 x1 exp(log_s) + c2];  dA[p][0:n_in] = [dx0, dx1 exp(log_s)];  d_skip[p] = end_w^T . de;
 * and per workgroup the partial sums [d_end_w (n_in C) | d_end_b (n_in) | d_start_w (C n_out/2) | d_start_b (C) | d_mix
 * (n_out^2)] at partial + workgroup * npart (the parts of a NULL end_w / mix_w are absent; npart is their exact total).
 * end_w NULL: the first call (the waveform; dx is dropped); mix_w NULL: the last call (n_emit == n_in). */
int t2amd_wg_head_bwd_rows(void);
int t2amd_wg_head_bwd_f32(const float* skip, long long ldskip, int C, const float* end_w, int n_in, const float* log_s,
                          long long lsb, long long lsc, const float* a_in, long long ldain, const float* x_sv, long long ldx,
                          const float* a_sv, long long ldasv, float* dA, long long lddA, const float* dh0, long long lddh,
                          const float* mix_w, const float* start_w, int n_emit, float* d_skip, long long ldds, float* partial,
                          long long npart, const int* rowb, const int* rowr, long long P, int n_group, int B, long long R,
                          float c1, float c2, void* stream);
/* out[i] = sum over blk < nblk, in that order, of partial[blk * n + i]. */
int t2amd_wg_partial_sum_f32(const float* partial, long long nblk, long long n, float* out, void* stream);
/* Gate backward on rows with rowb[m] >= 0 (others are not written), gate[m] = [t (C) | s (C)] as mode 0 kept them:
 * d_pre[m][c] = d_acts[m][c] s (1 - t^2);  d_pre[m][C + c] = d_acts[m][c] t s (1 - s);  acts[m][c] = t s. */
int t2amd_wg_gate_bwd_f32(const float* d_acts, long long ldd, const float* gate, long long ldg, const int* rowb, long long M,
                          int C, float* d_pre, long long ldp, float* acts, long long lda, void* stream);
/* Weight norm over a segment table (csrc/waveglow_wn.hip), one launch for all weight-normed tensors of a WaveGlow.
 * table: int64 [n_seg][6] on the device, per tensor {off, goff, dwoff, rows, len, first}: offsets in floats of the tensor
 * in the v / w / dv buffers (off), of its rows in the g / norm / dg buffers (goff) and of its gradient in the dw buffer
 * (dwoff), its rows and floats per row, and its first work unit (one unit per row when len >
 * t2amd_wg_weight_norm_short(), else one per 64 rows; counted through the table, n_units in all).  The caller
 * guarantees that every line lies inside the buffers; the bases are 16-byte aligned.
 *   fold:     n = sqrt(sum_j v[r][j]^2);  w[r][j] = v[r][j] (g[r] / n);  norm[r] = n
 *   backward: d = sum_j dw[r][j] v[r][j];  dg[r] = scale d / n;  dv[r][j] = scale (g[r] / n) (dw[r][j] - v[r][j] d / n^2)
 * The sum order of a row depends on len alone (fixed in-wave reduction, no atomics). */
int t2amd_wg_weight_norm_short(void);
int t2amd_wg_weight_norm_f32(const long long* table, int n_seg, long long n_units, const float* v_base, const float* g_base,
                             float* w_base, float* norm_base, void* stream);
int t2amd_wg_weight_norm_bwd_f32(const long long* table, int n_seg, long long n_units, const float* dw_base,
                                 const float* v_base, const float* g_base, const float* norm_base, float* dg_base,
                                 float* dv_base, float scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Optimiser step: global-norm clipping + Adam over all parameter
 * tensors in two launches.  Replaces reference train.py:233-236
 *   grad_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip_thresh)
 *   optimizer.step()                      # torch.optim.Adam(lr, weight_decay), train.py:170-171
 * with torch's arithmetic (L2 weight decay folded into the gradient, bias-corrected moments,
 * no amsgrad).  The state tensors (exp_avg, exp_avg_sq) are the ones torch.optim.Adam keeps, so
 * the reference's checkpoint format (train.py:112-118) is unchanged.
 * ------------------------------------------------------------------------------------ */
/* Tacotron2Loss (reference loss_function.py:8-19): loss = mean((mel - y)^2) + mean((mel_post - y)^2) +
 * mean(bce_with_logits(gate, g)) over the padded tensors, one reduction pass (fixed summation order, double partial sums:
 * bit-reproducible) and one gradient pass.  out4 = {total, mel term, postnet term, gate term}; ws holds
 * t2amd_loss_workspace_doubles() doubles; `upstream` is the device scalar d(total)/d(loss) (no host read). */
int t2amd_loss_workspace_doubles(void);
int t2amd_tacotron2_loss_fwd_f32(const float* mel, const float* mel_post, const float* mel_target, long long n_mel,
                                 const float* gate, const float* gate_target, long long n_gate, double* ws, float* out4,
                                 void* stream);
int t2amd_tacotron2_loss_bwd_f32(const float* mel, const float* mel_post, const float* mel_target, long long n_mel,
                                 const float* gate, const float* gate_target, long long n_gate, const float* upstream,
                                 float* d_mel, float* d_mel_post, float* d_gate, void* stream);

#define T2AMD_MAX_TENSORS 64
typedef struct t2amd_tensor_list {
    void* param[T2AMD_MAX_TENSORS];        /* f32, updated in place (unused by t2amd_grad_norm_f32) */
    const void* grad[T2AMD_MAX_TENSORS];   /* f32, read only: the clip factor is applied on the fly, p.grad is NOT rescaled */
    void* exp_avg[T2AMD_MAX_TENSORS];      /* f32 first moment */
    void* exp_avg_sq[T2AMD_MAX_TENSORS];   /* f32 second moment */
    long long numel[T2AMD_MAX_TENSORS];
    int first_block[T2AMD_MAX_TENSORS];    /* running sum of ceil(numel / t2amd_optim_chunk()) */
    int count;
} t2amd_tensor_list;

typedef struct t2amd_adam_hyper {
    float step_size;        /* lr / (1 - beta1^step) */
    float bc2_sqrt;         /* sqrt(1 - beta2^step) */
    float one_minus_beta1;
    float beta2;
    float one_minus_beta2;
    float eps;
    float weight_decay;     /* L2: g += weight_decay * p */
} t2amd_adam_hyper;

/* elements one workgroup covers (4096): callers size first_block[] and the workspace with it */
int t2amd_optim_chunk(void);
/* norm_and_coef[0] = ||all gradients||_2, [1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0).
 * ws: >= total blocks doubles.  Deterministic (fixed summation order). */
int t2amd_grad_norm_f32(const t2amd_tensor_list* L, float max_norm, double* ws, float* norm_and_coef, void* stream);
/* One Adam step on every tensor of the list; gradients are scaled by norm_and_coef[1] when the pointer is non-NULL. */
int t2amd_adam_step_f32(const t2amd_tensor_list* L, const t2amd_adam_hyper* h, const float* norm_and_coef,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * HiFi-GAN generator, inference (csrc/hifigan.hip, csrc/hifigan_post.hip; tacotron2_amd/hifigan.py).  The arithmetic is
 * restated in tests/hifigan_ref.py.  Channel-last row images X [P][C] f32.  The frame-rate row space packs the utterances
 * between zero halos of H0 rows, [H0 | n_0 | H0 | ... | n_{B-1} | H0]; rowb0[f] is the utterance of frame-level row f (-1 in
 * a halo), rowr0[f] its frame.  A stage with S times as many rows uses exactly that space times S: packed row p belongs to
 * frame-level row p / rdiv with rdiv = S, so P is a multiple of rdiv and n_rowb >= P / rdiv.  Every entry writes all rows of
 * its output and writes zero on rows whose rowb0 is negative; operand rows outside [0, P) read as zero.  The *_floats
 * arguments are the lengths of the buffers from the pointer on; an entry refuses a buffer shorter than the rows it
 * addresses.  precision 0 exact f32, 1 split-bf16 x3, 2 bf16.
 * ------------------------------------------------------------------------------------ */
/* out[m][n] = epi(bias[n] + sum_(tap, c) a(X[m + (tap - (taps-1)/2) dil][c]) W[n][tap Cin + c]) for all m < P, n < N;
 * a = leaky-ReLU(slope) when act, else identity.  epi: v = . (+ res[m][n] when res); v *= scale;
 * out = accumulate ? out + v : v.  res may be out (each element is read, then written, by the same lane).
 * Cin and N multiples of 32, at most 512; X and W 16-byte aligned, ldx a multiple of 4; taps odd. */
int t2amd_hg_conv_f32(const float* X, long long x_floats, long long ldx, long long P, int Cin, const float* W,
                      long long w_floats, const float* bias, int N, int taps, int dil, int act, float slope,
                      const float* res, long long ldres, long long res_floats, float* out, long long ldout,
                      long long out_floats, float scale, int accumulate, const int* rowb0, long long n_rowb, int rdiv,
                      int precision, void* stream);
/* ConvTranspose1d(Cin, N, ku, stride u, padding (ku - u) / 2) as u polyphase products in one launch: for every input row
 * m < P and phase ph < u, with q = ph + (ku - u) / 2,
 *   out[u m + ph][n] = bias[n] + sum_(j < ku / u, c) a(X[m + q / u - j][c]) W[ph][n][j Cin + c],
 * W[ph][n][j Cin + c] = weight[c][n][q % u + u j].  rdiv is that of the INPUT rows; out has u P rows.  ku a multiple of u,
 * ku - u even, u <= 64. */
int t2amd_hg_upsample_f32(const float* X, long long x_floats, long long ldx, long long P, int Cin, const float* W,
                          long long w_floats, const float* bias, int N, int ku, int u, int act, float slope, float* out,
                          long long ldout, long long out_floats, const int* rowb0, long long n_rowb, int rdiv,
                          int precision, void* stream);
/* conv_post: out[b T + rowr0[f] rdiv + p % rdiv] = tanh(bias[0] + sum_(tap < 7, c < C) lrelu(X[p + tap - 3][c]) w[tap C + c])
 * for the rows p < P whose f = p / rdiv has b = rowb0[f] >= 0 (other samples of out are not written).  C <= 64. */
int t2amd_hg_post_f32(const float* X, long long x_floats, long long ldx, long long P, int C, const float* w,
                      long long w_floats, const float* bias, float slope, const int* rowb0, const int* rowr0,
                      long long n_rowb, int rdiv, float* out, long long T, long long out_floats, void* stream);
/* out[f][c] = mel[b][c][rowr0[f]] for c < n_mel on rows with b = rowb0[f] >= 0, else 0 (f < P0, c < ldo); mel (B, n_mel, N)
 * contiguous. */
int t2amd_hg_pack_mel_f32(const float* mel, long long mel_floats, int B, int n_mel, long long N, const int* rowb0,
                          const int* rowr0, long long P0, float* out, int ldo, long long out_floats, void* stream);

/* ------------------------------------------------------------------------------------
 * Vocos vocoder, inference (csrc/vocos.hip, csrc/vocos_rows.hip; tacotron2_amd/vocos.py).  The arithmetic is restated in
 * tests/vocos_ref.py.  Everything runs at the frame rate, in the frame-level packed row space of the HiFi-GAN block above
 * with H0 = 3: [3 | n_0 | 3 | ... | n_{B-1} | 3], rowb0[p] the utterance of packed row p (-1 in a halo), n_rowb >= P.  Every
 * entry writes all rows of its output and writes zero on rows whose rowb0 is negative; operand rows outside [0, P) read as
 * zero.  The *_floats arguments are the lengths of the buffers from the pointer on; an entry refuses a buffer shorter than
 * the rows it addresses.  precision 0 exact f32, 1 split-bf16 x3, 2 bf16.
 * ------------------------------------------------------------------------------------ */
/* Depthwise convolution plus LayerNorm over the D channels of every row, one launch:
 *   y[p][c] = conv_bias[c] + sum_(t < taps) X[p + t - (taps-1)/2][c] w[t D + c]     (taps = 0: y = X, w and conv_bias unused)
 *   out[p][c] = (y[p][c] - mean_c y[p]) / sqrt(var_c y[p] + eps) ln_w[c] + ln_b[c]  (biased variance)
 * D a multiple of 32, at most 512; taps 0 or odd, at most 15; all operands 16-byte aligned, ldx and ldout multiples of 4;
 * out must not be X. */
int t2amd_vc_dwln_f32(const float* X, long long x_floats, long long ldx, long long P, int D, const float* w,
                      long long w_floats, const float* conv_bias, int taps, const float* ln_w, const float* ln_b, float eps,
                      const int* rowb0, long long n_rowb, float* out, long long ldout, long long out_floats, void* stream);
/* out[m][n] = epi(bias[n] + sum_(k < K) X[m][k] W[n K + k]) for all m < P, n < N.  epi 0: v; 1: exact GELU
 * v (1 + erf(v / sqrt 2)) / 2; 2: res[m][n] + gamma[n] v (res may be out: each element is read, then written, by the same
 * lane).  bias may be NULL for epi 0 and 1.  K and N multiples of 32, at most 16416; X and W 16-byte aligned, ldx a multiple
 * of 4; out must not be X. */
int t2amd_vc_linear_f32(const float* X, long long x_floats, long long ldx, long long P, int K, const float* W,
                        long long w_floats, const float* bias, int N, int epi, const float* gamma, const float* res,
                        long long ldres, long long res_floats, float* out, long long ldout, long long out_floats,
                        const int* rowb0, long long n_rowb, int precision, void* stream);
/* Head rows Y[p] = [m_0 .. m_{F-1} | ph_0 .. ph_{F-1}] -> interleaved complex rows:
 *   S[p][2k, 2k+1] = min(exp(m_k), clamp) (cos ph_k, sin ph_k) for k < F;  zero for F <= k < lds / 2.  lds even. */
int t2amd_vc_polar_f32(const float* Y, long long y_floats, long long ldy, long long P, int F, float clamp, const int* rowb0,
                       long long n_rowb, float* S, long long lds, long long s_floats, void* stream);
/* Overlap-add of windowed inverse-transform frames (L samples a row) into out (B, T).  utt (int32, device) holds
 * [first packed row, frames n_b] of every utterance.  For t < hop (n_b - 1) + L - 2 trim, with s = t + trim,
 *   out[b][t] = sum_j frames[row_b + j][s - j hop] / sum_j wsq[s - j hop]   over the frames 0 <= j < n_b that cover s,
 * in ascending j; out[b][t] = 0 beyond.  wsq[L] is the squared window.  hop divides L, (L - hop) / 2 <= trim <= L / 2
 * (Vocos' 'same' and 'center' paddings); B at most 65535. */
int t2amd_vc_ola_f32(const float* frames, long long f_floats, long long ldf, long long P, const float* wsq, const int* utt,
                     int B, int L, int hop, int trim, float* out, long long T, long long out_floats, void* stream);

/* ------------------------------------------------------------------------------------
 * Vocos vocoder, the row kernels of the backward pass (csrc/vocos_bwd.hip; Vocos.generate).  The dense data gradients are
 * t2amd_vc_linear_f32 against transposed weight images, the weight gradients t2amd_gemm_f32.  Same row space and rules as
 * above: every entry writes all rows of its outputs and zero on halo rows.  A sum over rows leaves as partial slots, one
 * per t2amd_vc_bwd_slot_rows() consecutive rows (slot s covers rows [s rows, (s + 1) rows)); t2amd_wg_partial_sum_f32 adds
 * the ceil(P / rows) slots in order, so two calls give the same bits.  All images 16-byte aligned, row strides multiples
 * of 4, D a multiple of 32 up to 512.
 * ------------------------------------------------------------------------------------ */
int t2amd_vc_bwd_slot_rows(void);
/* d_frames[p][t] = d_audio[b][s - trim] / sum_j wsq[s - j hop] with b = rowb0[p], s = rowr0[p] hop + t, where 0 <= s - trim <
 * min(T, hop (n_b - 1) + L - 2 trim); zero elsewhere and on halo rows.  The sum is t2amd_vc_ola_f32's.  L a multiple of 4. */
int t2amd_vc_ola_bwd_f32(const float* d_audio, long long T, long long a_floats, const float* wsq, const int* utt, int B,
                         const int* rowb0, const int* rowr0, long long n_rowb, long long P, int L, int hop, int trim,
                         float* d_frames, long long ldf, long long f_floats, void* stream);
/* From Y[p] = [m | ph] and d_S[p] = interleaved (d_re, d_im), with e = exp m, mag = min(e, clamp):
 *   d_Y[p][k] = e <= clamp ? mag (cos ph d_re + sin ph d_im) : 0,  d_Y[p][F + k] = mag (cos ph d_im - sin ph d_re),
 * zero in the columns 2 F <= c < N. */
int t2amd_vc_polar_bwd_f32(const float* Y, long long y_floats, long long ldy, long long P, int F, float clamp, const float* dS,
                           long long ds_floats, long long lds, const int* rowb0, long long n_rowb, float* dY, long long lddy,
                           long long dy_floats, int N, void* stream);
/* d_H[p][c] *= Phi(U[p][c]) + U[p][c] phi(U[p][c]) (the derivative of the exact GELU), in place; I a multiple of 32. */
int t2amd_vc_gelu_bwd_f32(const float* U, long long u_floats, long long ldu, long long P, int I, const int* rowb0,
                          long long n_rowb, float* dH, long long ldh, long long dh_floats, void* stream);
/* partial[slot][c] = sum_r d_X[r][c] Y2[r][c], then Y2[r][c] = gamma[c] d_X[r][c] (in place). */
int t2amd_vc_gamma_bwd_f32(const float* dX, long long dx_floats, long long lddx, long long P, int D, const float* gamma,
                           const int* rowb0, long long n_rowb, float* Y2, long long ldy, long long y_floats, float* partial,
                           long long partial_floats, void* stream);
/* Backward of t2amd_vc_dwln_f32's LayerNorm with G = d_out: y and xh = (y - mean) rstd are recomputed from X (w, conv_bias,
 * taps as in the forward; taps at most 7 here),
 *   d_Z[p][c] = rstd (ln_w[c] G[p][c] - mean_c(ln_w G[p]) - xh[p][c] mean_c(ln_w G[p] xh[p])),
 *   partial[slot] = [sum_r G[r][c] xh[r][c] (D) | sum_r G[r][c] (D)].   d_Z may be G, must not be X. */
int t2amd_vc_ln_bwd_f32(const float* X, long long x_floats, long long ldx, long long P, int D, const float* w, long long w_floats,
                        const float* conv_bias, int taps, const float* ln_w, float eps, const int* rowb0, long long n_rowb,
                        const float* G, long long ldg, long long g_floats, float* dZ, long long lddz, long long dz_floats,
                        float* partial, long long partial_floats, void* stream);
/* Backward of the depthwise convolution over the finished d_Z image, half = (taps - 1) / 2:
 *   d_X[p][c] = res[p][c] + sum_t w[t D + c] d_Z[p + half - t][c]    (res may be NULL or d_X)
 *   partial[slot] = [sum_r d_Z[r][c] X[r + t - half][c] (taps x D) | sum_r d_Z[r][c] (D)].   d_X must not be d_Z or X. */
int t2amd_vc_dw_bwd_f32(const float* dZ, long long dz_floats, long long lddz, long long P, int D, const float* X,
                        long long x_floats, long long ldx, const float* w, long long w_floats, int taps, const int* rowb0,
                        long long n_rowb, const float* res, long long ldres, long long res_floats, float* dX, long long lddx,
                        long long dx_floats, float* partial, long long partial_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TACOTRON2_AMD_H */
