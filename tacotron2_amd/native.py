"""ctypes binding of ``libtacotron2_amd.so`` (C ABI: ``include/tacotron2_amd.h``).

The engine has exactly one compute path: the HIP kernels behind this module.
There is no CPU or eager-PyTorch fallback — if the library is missing or a
tensor is not a device tensor the call fails loudly.  PyTorch is used for
device memory and streams only: every wrapper takes ``torch`` tensors, checks
dtype/layout, and hands raw device pointers plus the current HIP stream to the
library.

Build the library with ``python -m tacotron2_amd.build`` (hipcc, gfx950).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("T2AMD_LIB", os.path.join(_HERE, "lib", "libtacotron2_amd.so"))

TORCH_OPS_PATH = os.path.join(_HERE, "lib", "libtacotron2_amd_torch.so")

ATT_DIM = 128
LOC_FILTERS = 32
LOC_KERNEL = 31
LOC_TAPS = 62
ATT_SLICES = 4

_f32p = C.c_void_p
_i64 = C.c_longlong


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", _f32p), ("B", _f32p), ("C", _f32p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("lda", _i64), ("ldb", _i64), ("ldc", _i64),
        ("a_kcontig", C.c_int), ("b_kcontig", C.c_int),
        ("batch", C.c_int),
        ("strideA", _i64), ("strideB", _i64), ("strideC", _i64),
        ("splitk", C.c_int), ("strideSplitC", _i64),
        ("accumulate", C.c_int),
        ("bias", _f32p), ("act", C.c_int),
        ("keep", C.c_void_p), ("ldkeep", _i64), ("keep_scale", C.c_float),
        ("convA_T", C.c_int), ("convA_C", C.c_int), ("convA_pad", C.c_int), ("convA_sign", C.c_int),
        ("convB_T", C.c_int), ("convB_C", C.c_int), ("convB_pad", C.c_int),
        ("precision", C.c_int),
    ]


class Gemm16Desc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", _f32p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("lda", _i64), ("ldb", _i64), ("ldc", _i64),
        ("splitk", C.c_int), ("strideSplitC", _i64), ("accumulate", C.c_int), ("bias", _f32p),
        ("win_T", C.c_int), ("win_Tp", C.c_int),
    ]


class Seg(C.Structure):
    _fields_ = [("p", _f32p), ("ld", _i64), ("width", C.c_int)]


class LstmStep(C.Structure):
    _fields_ = [
        ("x", Seg * 3), ("nseg", C.c_int),
        ("W", _f32p), ("Ktot", C.c_int), ("H", C.c_int), ("B", C.c_int),
        ("gin", _f32p), ("ld_gin", _i64),
        ("bias", _f32p),
        ("c_prev", _f32p), ("ld_cprev", _i64),
        ("gates_out", _f32p), ("ld_gates", _i64),
        ("c_out", _f32p), ("ld_c", _i64),
        ("h_out", _f32p), ("ld_h", _i64),
        ("keep", C.c_void_p), ("ld_keep", _i64), ("keep_scale", C.c_float),
        ("lens", C.c_void_p), ("t", C.c_int), ("tag", C.c_int),
        ("bf16", C.c_int), ("h16_out", C.c_void_p), ("ld_h16", _i64),
    ]


class SkinnyGemm(C.Structure):
    _fields_ = [
        ("x", Seg * 3), ("nseg", C.c_int),
        ("W", _f32p), ("Ktot", C.c_int), ("N", C.c_int), ("B", C.c_int),
        ("Y", _f32p), ("ldy", _i64), ("nsplit", C.c_int), ("split_stride", _i64), ("tag", C.c_int),
        ("bf16", C.c_int),
        ("bias", _f32p), ("act", C.c_int), ("keep", C.c_void_p), ("ld_keep", _i64), ("keep_scale", C.c_float),
        ("Y16", C.c_void_p), ("ldy16", _i64),
        ("stop_active", C.c_void_p), ("stop_lengths", C.c_void_p), ("stop_done", C.c_void_p),
        ("stop_col", C.c_int), ("stop_t", C.c_int), ("stop_max_steps", C.c_int), ("stop_threshold", C.c_float),
    ]


class Addend(C.Structure):
    _fields_ = [("p", _f32p), ("ld", _i64), ("nsplit", C.c_int), ("split_stride", _i64)]


class LstmBwd(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("H", C.c_int),
        ("dh", Addend * 3),
        ("gates", _f32p), ("ld_gates", _i64),
        ("c_prev", _f32p), ("ld_cprev", _i64),
        ("c", _f32p), ("ld_c", _i64),
        ("keep", C.c_void_p), ("ld_keep", _i64), ("keep_scale", C.c_float),
        ("dc", _f32p), ("ld_dc", _i64),
        ("dgates", _f32p), ("ld_dgates", _i64),
        ("lens", C.c_void_p), ("t", C.c_int),
        ("dgates16", C.c_void_p), ("ld_dgates16", _i64),
        ("dgates16_x3", C.c_int),
    ]


class AttnFwd(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("Ti", C.c_int), ("E", C.c_int), ("Hq", C.c_int),
        ("h", _f32p), ("ld_h", _i64),
        ("Wq", _f32p), ("U", _f32p), ("v", _f32p), ("pm", _f32p), ("memory", _f32p),
        ("lens", C.c_void_p),
        ("w_prev", _f32p), ("ld_wprev", _i64),
        ("cum", _f32p), ("cum_save", _f32p),
        ("w_out", _f32p), ("ld_wout", _i64),
        ("ctx_out", _f32p), ("ld_ctx", _i64),
        ("q_out", _f32p), ("ld_q", _i64),
        ("active", C.c_void_p),
        ("ws", _f32p),
        ("ctx16_out", C.c_void_p), ("ld_ctx16", _i64),
        ("loc_split_bf16", C.c_int),
        ("memory16", C.c_void_p),
        ("Wq16", C.c_void_p),
        ("ws_floats", _i64),
        ("ctx16_x3", C.c_int),
    ]


class AttnBwd(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("Ti", C.c_int), ("E", C.c_int), ("Hq", C.c_int),
        ("dctx", Addend * 3),
        ("dctx_total", _f32p), ("ld_dctx_total", _i64),
        ("d_w_extra", _f32p), ("ld_dwextra", _i64),
        ("q", _f32p), ("ld_q", _i64),
        ("Wq", _f32p), ("U", _f32p), ("v", _f32p), ("pm", _f32p), ("memory", _f32p),
        ("lens", C.c_void_p),
        ("w", _f32p), ("ld_w", _i64),
        ("w_prev", _f32p), ("ld_wprev", _i64),
        ("cum_before", _f32p),
        ("dwin_part", _f32p), ("dcum_acc", _f32p),
        ("d_pm", _f32p), ("dU_acc", _f32p), ("dv_acc", _f32p),
        ("dq_out", _f32p), ("ld_dq", _i64),
        ("dh_out", _f32p), ("ld_dh", _i64), ("dh_split_stride", _i64),
        ("ws", _f32p),
        ("bf16", C.c_int),
        ("memory16", C.c_void_p),
        ("cell_q", C.POINTER(LstmBwd)), ("cell_x", C.POINTER(LstmBwd)),
        ("ws_floats", _i64),
        ("Wq16", C.c_void_p),
    ]


class DecTrain(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("Ti", C.c_int), ("To", C.c_int), ("E", C.c_int), ("Ha", C.c_int), ("Hd", C.c_int),
        ("Wa_rec", _f32p), ("Wd_cat", _f32p), ("bias_d", _f32p), ("Wq", _f32p), ("U", _f32p), ("v", _f32p),
        ("GA", _f32p), ("memory", _f32p), ("pm", _f32p), ("lens", C.c_void_p),
        ("keep_att", C.c_void_p), ("keep_dec", C.c_void_p),
        ("scale_att", C.c_float), ("scale_dec", C.c_float),
        ("HA", _f32p), ("CA", _f32p), ("GD", _f32p), ("HD", _f32p), ("CD", _f32p), ("CTX", _f32p),
        ("Q", _f32p), ("ALIGN", _f32p), ("CUM", _f32p), ("cum_work", _f32p), ("attn_ws", _f32p),
        ("bf16", C.c_int), ("Wa_rec16", C.c_void_p), ("Wd_cat16", C.c_void_p),
        ("HA16", C.c_void_p), ("HD16", C.c_void_p), ("CTX16", C.c_void_p),
        ("memory16", C.c_void_p), ("Wq16", C.c_void_p),
    ]


class DecTrainBwd(C.Structure):
    _fields_ = [
        ("f", DecTrain),
        ("Wa_recT", _f32p), ("Wd_catT", _f32p), ("DHC", _f32p), ("d_align", _f32p),
        ("nsplit", C.c_int),
        ("DGA", _f32p), ("DGD", _f32p), ("DCTX", _f32p), ("DQ", _f32p), ("d_pm", _f32p),
        ("dU_acc", _f32p), ("dv_acc", _f32p),
        ("dXd", _f32p), ("dXa", _f32p), ("dc_a", _f32p), ("dc_d", _f32p),
        ("dwin_part", _f32p), ("dcum_acc", _f32p), ("dq_h", _f32p),
        ("Wa_recT16", C.c_void_p), ("Wd_catT16", C.c_void_p), ("DGA16", C.c_void_p), ("DGD16", C.c_void_p),
        ("dg16_step_a", _i64), ("dg16_step_d", _i64),
        ("dXd_ring", C.c_int),
    ]


class LstmSeq(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("T", C.c_int), ("H", C.c_int), ("reverse", C.c_int),
        ("Whh", _f32p), ("WhhT", _f32p), ("GX", _f32p),
        ("out", _f32p), ("ld_out", _i64),
        ("C", _f32p), ("lens", C.c_void_p),
        ("dout", _f32p), ("ld_dout", _i64),
        ("DG", _f32p), ("dX", _f32p), ("dc", _f32p),
        ("dx_splits", C.c_int),
    ]


class SmallLinear(C.Structure):
    _fields_ = [
        ("X", _f32p), ("ldx", _i64), ("W", _f32p), ("ldw", _i64), ("bias", _f32p),
        ("Y", _f32p), ("ldy", _i64),
        ("B", C.c_int), ("N", C.c_int), ("K", C.c_int), ("act", C.c_int),
        ("keep", C.c_void_p), ("ldkeep", _i64), ("keep_scale", C.c_float),
    ]


class DecInfer(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("Ti", C.c_int), ("E", C.c_int), ("Ha", C.c_int), ("Hd", C.c_int),
        ("P", C.c_int), ("C", C.c_int),
        ("t0", C.c_int), ("n_steps", C.c_int), ("max_steps", C.c_int),
        ("gate_threshold", C.c_float),
        ("W1", _f32p), ("W2", _f32p), ("Wa_cat", _f32p), ("bias_a", _f32p), ("Wd_cat", _f32p),
        ("bias_d", _f32p), ("Wq", _f32p), ("U", _f32p), ("v", _f32p), ("Wpg", _f32p), ("bias_pg", _f32p),
        ("memory", _f32p), ("pm", _f32p), ("lens", C.c_void_p), ("keep_prenet", C.c_void_p),
        ("h_a", _f32p), ("c_a", _f32p), ("c_d", _f32p), ("hc", _f32p), ("cum", _f32p),
        ("x_prenet", _f32p), ("gates", _f32p), ("zero_frame", _f32p), ("attn_ws", _f32p),
        ("PG", _f32p), ("ALIGN", _f32p), ("out_lengths", C.c_void_p), ("active", C.c_void_p),
        ("done_count", C.c_void_p),
        ("bf16", C.c_int), ("Wa_cat16", C.c_void_p), ("Wd_cat16", C.c_void_p),
        ("x_prenet16", C.c_void_p), ("h_a16", C.c_void_p), ("hc16", C.c_void_p),
        ("Wf", _f32p), ("bias_f", _f32p), ("memory16", C.c_void_p), ("Wq16", C.c_void_p),
        ("Wf16", C.c_void_p), ("Wpg16", C.c_void_p), ("W2_16", C.c_void_p), ("x_prenet1_16", C.c_void_p),
        ("attn_ws_floats", _i64),
    ]


class DecPersist(C.Structure):
    _fields_ = [
        ("Ti", C.c_int), ("E", C.c_int), ("H", C.c_int), ("P", C.c_int), ("C", C.c_int),
        ("max_steps", C.c_int), ("gate_threshold", C.c_float),
        ("Wa16", C.c_void_p), ("Wd16", C.c_void_p), ("bias_a", _f32p), ("bias_d", _f32p),
        ("Wq", _f32p), ("U", _f32p), ("v", _f32p), ("Wf", _f32p), ("bias_f", _f32p), ("W2", _f32p),
        ("memory", _f32p), ("pm", _f32p), ("keep_prenet", C.c_void_p),
        ("PG", _f32p), ("ALIGN", _f32p), ("out_length", C.c_void_p), ("status", C.c_void_p),
        ("steps_done", C.c_void_p), ("mailbox", C.c_void_p), ("trace", _f32p), ("timing", C.c_void_p),
        ("weights_f32", C.c_int),
    ]


PERSIST_TIMEOUT = 7
MAX_TENSORS = 64


class TensorList(C.Structure):
    _fields_ = [("param", C.c_void_p * MAX_TENSORS), ("grad", C.c_void_p * MAX_TENSORS),
                ("exp_avg", C.c_void_p * MAX_TENSORS), ("exp_avg_sq", C.c_void_p * MAX_TENSORS),
                ("numel", C.c_longlong * MAX_TENSORS), ("first_block", C.c_int * MAX_TENSORS), ("count", C.c_int)]


class AdamHyper(C.Structure):
    _fields_ = [("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("one_minus_beta1", C.c_float),
                ("beta2", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float)]


_STRUCTS = [GemmDesc, Seg, LstmStep, SkinnyGemm, Addend, LstmBwd, AttnFwd, AttnBwd, DecTrain,
            DecTrainBwd, LstmSeq, DecInfer, SmallLinear, TensorList, AdamHyper, DecPersist, Gemm16Desc]

# every exported symbol of include/tacotron2_amd.h
SYMBOLS = [
    "t2amd_abi_version", "t2amd_source_sha1", "t2amd_last_error", "t2amd_struct_sizes", "t2amd_set_validate_only", "t2amd_profile_enable", "t2amd_profile_read", "t2amd_profile_event_overhead",
    "t2amd_gemm_f32", "t2amd_gemm_tile_size", "t2amd_splitk_reduce_f32", "t2amd_splitk_reduce2d_f32", "t2amd_gemm16_tn", "t2amd_gemm16_kk", "t2amd_gemm16_kk_group", "t2amd_transpose_cast_bf16", "t2amd_cast_halo_bf16", "t2amd_pack_conv_bf16",
    "t2amd_bn_stats_f32", "t2amd_bn_eval_invstd_f32", "t2amd_bn_act_fwd_f32", "t2amd_bn_act_bwd_f32", "t2amd_bn_act_bwd_img_f32", "t2amd_colsum_bf16", "t2amd_bn_act_fwd_img_f32",
    "t2amd_colsum_f32",
    "t2amd_embedding_fwd_f32", "t2amd_embedding_bwd_f32", "t2amd_philox_keep_mask", "t2amd_fill_f32",
    "t2amd_copy2d_f32", "t2amd_cast_bf16_f32", "t2amd_split_bf16x3_f32", "t2amd_transpose_f32", "t2amd_frames_to_time_major_f32",
    "t2amd_split_projection_f32", "t2amd_finalize_outputs_f32", "t2amd_grads_to_channel_last_f32",
    "t2amd_gather_dout_f32", "t2amd_relu_dropout_bwd_f32",
    "t2amd_lstm_step_fwd_f32", "t2amd_skinny_gemm_f32", "t2amd_lstm_pointwise_bwd_f32",
    "t2amd_lstm_step_fwd2_f32", "t2amd_skinny_gemm2_f32", "t2amd_lstm_pointwise_bwd2_f32",
    "t2amd_fold_location_f32", "t2amd_unfold_location_grads_f32",
    "t2amd_attention_step_fwd_f32", "t2amd_attention_step_bwd_f32",
    "t2amd_decoder_train_fwd_loop_f32", "t2amd_decoder_train_bwd_loop_f32",
    "t2amd_decoder_train_fwd_persistent_flag_bytes", "t2amd_decoder_train_fwd_persistent_supported", "t2amd_decoder_train_fwd_persistent_f32",
    "t2amd_lstm_seq_fwd_f32", "t2amd_lstm_seq_bwd_f32", "t2amd_decoder_infer_steps_f32",
    "t2amd_set_decoder_streams", "t2amd_set_bptt_cell_fold", "t2amd_get_bptt_cell_fold", "t2amd_attn_bwd_ws_floats",
    "t2amd_set_small_batch_max", "t2amd_get_small_batch_max", "t2amd_dec_infer_uses_tiles",
    "t2amd_set_attn_bwd_granules", "t2amd_attn_handoff_timeouts", "t2amd_set_attn_bwd_fused", "t2amd_attn_fwd_ws_floats", "t2amd_set_attn_fwd_fused", "t2amd_lstm_step_small_f32", "t2amd_linear_small_f32",
    "t2amd_lstm_seq_fwd2_f32", "t2amd_lstm_seq_bwd2_f32",
    "t2amd_lstm_seq_persistent_mailbox_bytes", "t2amd_lstm_seq_persistent_supported", "t2amd_lstm_seq_fwd2_persistent_f32",
    "t2amd_lstm_seq_batch_persistent_flag_bytes", "t2amd_lstm_seq_batch_persistent_supported", "t2amd_lstm_seq_fwd2_batch_persistent_f32", "t2amd_encoder_handoff_timeouts",
    "t2amd_lstm_seq_bwd2_batch_persistent_supported", "t2amd_lstm_seq_bwd2_batch_persistent_f32",
    "t2amd_reflect_pad_f32", "t2amd_reflect_index", "t2amd_stft_magnitude_f32", "t2amd_mel_log_compress_f32",
    "t2amd_mel_log_bwd_f32", "t2amd_stft_magnitude_bwd_f32", "t2amd_stft_frames_fold_f32", "t2amd_mel_l1_rows_per_slot",
    "t2amd_mel_l1_fwd_f32", "t2amd_mel_l1_bwd_f32",
    "t2amd_stft_loss_rows_per_slot", "t2amd_stft_loss_fwd_f32", "t2amd_stft_loss_finish_f64", "t2amd_stft_loss_bwd_f32",
    "t2amd_stft_loss_sum_f32",
    "t2amd_resample_plan", "t2amd_resample_fwd_f32", "t2amd_resample_bwd_f32",
    "t2amd_dtw_width", "t2amd_mel_cepstrum_f32", "t2amd_dtw_f32", "t2amd_dtw_backtrack",
    "t2amd_yin_plan", "t2amd_yin_f32",
    "t2amd_align_limits", "t2amd_align_workspace", "t2amd_monotonic_align_f32",
    "t2amd_forward_sum_workspace", "t2amd_forward_sum_f32", "t2amd_forward_sum_bwd_f32",
    "t2amd_aligner_workspace", "t2amd_aligner_pack_keys_f32", "t2amd_aligner_transpose_f32", "t2amd_aligner_rows_fwd_f32",
    "t2amd_aligner_rows_bwd_f32", "t2amd_aligner_scores_f32", "t2amd_aligner_scores_bwd_f32", "t2amd_aligner_product_f32",
    "t2amd_beta_binomial_log_prior_f32",
    "t2amd_regulate_limits", "t2amd_durations_to_path_i32", "t2amd_length_regulate_f32", "t2amd_length_regulate_bwd_f32",
    "t2amd_token_average_f32", "t2amd_token_average_bwd_f32",
    "t2amd_self_attn_limits", "t2amd_self_attn_workspace", "t2amd_self_attn_f32", "t2amd_self_attn_delta_f32",
    "t2amd_self_attn_bwd_f32",
    "t2amd_fft_block_limits", "t2amd_fft_block_workspace", "t2amd_ffb_conv_f32", "t2amd_ffb_conv_dw_f32", "t2amd_ffb_transpose_f32",
    "t2amd_ffb_dw_finish_f32", "t2amd_ffb_add_ln_f32", "t2amd_ffb_add_ln_bwd_f32", "t2amd_ffb_colsum_f32", "t2amd_ffb_relu_mask_f32",
    "t2amd_predictor_limits", "t2amd_predictor_workspace", "t2amd_pred_project_f32", "t2amd_pred_project_bwd_f32",
    "t2amd_pred_project_sums_f32", "t2amd_pred_embed_f32", "t2amd_pred_embed_bwd_f32", "t2amd_pred_embed_sums_f32",
    "t2amd_gl_packed_rows", "t2amd_gl_overlap_add_f32", "t2amd_gl_project_f32", "t2amd_gl_rect_f32", "t2amd_stft_polar_f32",
    "t2amd_mel_decompress_f32",
    "t2amd_wg_layer_f32", "t2amd_wg_tail_f32", "t2amd_wg_denoise_f32", "t2amd_wg_head_f32", "t2amd_wg_nll_chunk", "t2amd_wg_nll_f32",
    "t2amd_wg_layer_train_f32", "t2amd_wg_head_save_f32", "t2amd_wg_head_bwd_rows", "t2amd_wg_head_bwd_f32",
    "t2amd_wg_partial_sum_f32", "t2amd_wg_gate_bwd_f32",
    "t2amd_wg_weight_norm_short", "t2amd_wg_weight_norm_f32", "t2amd_wg_weight_norm_bwd_f32",
    "t2amd_optim_chunk", "t2amd_grad_norm_f32", "t2amd_adam_step_f32",
    "t2amd_decoder_persist_mailbox_bytes", "t2amd_decoder_persist_supported", "t2amd_decoder_infer_persistent_f32",
    "t2amd_loss_workspace_doubles", "t2amd_tacotron2_loss_fwd_f32", "t2amd_tacotron2_loss_bwd_f32",
    "t2amd_hg_conv_f32", "t2amd_hg_upsample_f32", "t2amd_hg_post_f32", "t2amd_hg_pack_mel_f32",
    "t2amd_vc_dwln_f32", "t2amd_vc_linear_f32", "t2amd_vc_polar_f32", "t2amd_vc_ola_f32",
    "t2amd_vc_bwd_slot_rows", "t2amd_vc_ola_bwd_f32", "t2amd_vc_polar_bwd_f32", "t2amd_vc_gelu_bwd_f32", "t2amd_vc_gamma_bwd_f32",
    "t2amd_vc_ln_bwd_f32", "t2amd_vc_dw_bwd_f32",
]

_P, _I, _L, _F, _UL = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_ulonglong


def _argtypes():
    pt = C.POINTER
    return {
        "t2amd_gemm_f32": [pt(GemmDesc), _P],
        "t2amd_gemm_tile_size": [_I, _I, _I, _I, _I, _I],
        "t2amd_splitk_reduce_f32": [_P, _I, _L, _P, _L, _I, _I, _I, _P],
        "t2amd_splitk_reduce2d_f32": [_P, _I, _L, _P, _I, _I, _L, _I, _P],
        "t2amd_gemm16_tn": [pt(Gemm16Desc), _P],
        "t2amd_gemm16_kk": [pt(Gemm16Desc), _P],
        "t2amd_gemm16_kk_group": [pt(Gemm16Desc), _I, _P],
        "t2amd_transpose_cast_bf16": [_P, _I, _L, _P, _L, _I, _I, _I, _P],
        "t2amd_cast_halo_bf16": [_P, _L, _P, _L, _I, _I, _I, _P],
        "t2amd_pack_conv_bf16": [_P, _P, _I, _I, _I, _I, _I, _P],
        "t2amd_bn_stats_f32": [_P, _L, _I, _I, _P, _P, _P, _P, _P, _F, _F, _P],
        "t2amd_bn_eval_invstd_f32": [_P, _P, _I, _F, _P],
        "t2amd_bn_act_fwd_f32": [_P, _L, _P, _L, _I, _I, _P, _P, _P, _P, _I, _P, _L, _F, _P, _I, _P],
        "t2amd_bn_act_fwd_img_f32": [_P, _L, _P, _L, _I, _I, _P, _P, _P, _P, _I, _P, _L, _F, _P, _I, _I, _P],
        "t2amd_bn_act_bwd_f32": [_P, _L, _P, _L, _P, _L, _I, _I, _P, _P, _P, _I, _P, _L, _F, _P, _P, _P, _P],
        "t2amd_bn_act_bwd_img_f32": [_P, _L, _P, _L, _P, _L, _I, _I, _P, _P, _P, _I, _P, _L, _F, _P, _P, _P, _P, _I, _I, _P, _I, _P],
        "t2amd_colsum_f32": [_P, _L, _I, _I, _P, _P, _I, _P],
        "t2amd_colsum_bf16": [_P, _L, _I, _I, _P, _P, _I, _P],
        "t2amd_embedding_fwd_f32": [_P, _P, _P, _L, _I, _I, _P],
        "t2amd_embedding_bwd_f32": [_P, _P, _P, _P, _L, _I, _I, _P],
        "t2amd_philox_keep_mask": [_P, _L, _F, _UL, _UL, _P],
        "t2amd_fill_f32": [_P, _L, _F, _P],
        "t2amd_cast_bf16_f32": [_P, _P, _L, _P],
        "t2amd_split_bf16x3_f32": [_P, _L, _P, _L, _L, _I, _P],
        "t2amd_copy2d_f32": [_P, _L, _P, _L, _P, _L, _I, _I, _P],
        "t2amd_transpose_f32": [_P, _L, _P, _L, _I, _I, _I, _L, _L, _P],
        "t2amd_frames_to_time_major_f32": [_P, _P, _I, _I, _I, _P],
        "t2amd_split_projection_f32": [_P, _P, _P, _P, _I, _I, _I, _P],
        "t2amd_finalize_outputs_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
        "t2amd_grads_to_channel_last_f32": [_P, _P, _P, _P, _I, _I, _I, _P],
        "t2amd_gather_dout_f32": [_P, _P, _P, _I, _I, _I, _P],
        "t2amd_relu_dropout_bwd_f32": [_P, _P, _F, _L, _P],
        "t2amd_lstm_step_fwd_f32": [pt(LstmStep), _P],
        "t2amd_skinny_gemm_f32": [pt(SkinnyGemm), _P],
        "t2amd_lstm_pointwise_bwd_f32": [pt(LstmBwd), _P],
        "t2amd_lstm_step_fwd2_f32": [pt(LstmStep), pt(LstmStep), _P],
        "t2amd_skinny_gemm2_f32": [pt(SkinnyGemm), pt(SkinnyGemm), _P],
        "t2amd_lstm_pointwise_bwd2_f32": [pt(LstmBwd), pt(LstmBwd), _P],
        "t2amd_fold_location_f32": [_P, _P, _P, _P],
        "t2amd_unfold_location_grads_f32": [_P, _P, _I, _P, _P, _P, _P, _P, _P],
        "t2amd_attention_step_fwd_f32": [pt(AttnFwd), _P],
        "t2amd_attention_step_bwd_f32": [pt(AttnBwd), _P],
        "t2amd_decoder_train_fwd_loop_f32": [pt(DecTrain), _P],
        "t2amd_decoder_train_fwd_persistent_flag_bytes": [_I, _I],
        "t2amd_decoder_train_fwd_persistent_supported": [pt(DecTrain), _I],
        "t2amd_decoder_train_fwd_persistent_f32": [pt(DecTrain), _P, _P, _P, _P],
        "t2amd_decoder_train_bwd_loop_f32": [pt(DecTrainBwd), _P],
        "t2amd_lstm_seq_fwd_f32": [pt(LstmSeq), _P],
        "t2amd_lstm_seq_bwd_f32": [pt(LstmSeq), _P],
        "t2amd_lstm_seq_fwd2_f32": [pt(LstmSeq), pt(LstmSeq), _P],
        "t2amd_lstm_seq_bwd2_f32": [pt(LstmSeq), pt(LstmSeq), _P],
        "t2amd_lstm_seq_persistent_mailbox_bytes": [_I, _I],
        "t2amd_lstm_seq_persistent_supported": [pt(LstmSeq)],
        "t2amd_lstm_seq_fwd2_persistent_f32": [pt(LstmSeq), pt(LstmSeq), _P, _P, _P],
        "t2amd_lstm_seq_batch_persistent_flag_bytes": [_I, _I, _I],
        "t2amd_lstm_seq_batch_persistent_supported": [pt(LstmSeq), _I, _I],
        "t2amd_lstm_seq_fwd2_batch_persistent_f32": [pt(LstmSeq), pt(LstmSeq), _P, _P, _P, _P],
        "t2amd_lstm_seq_bwd2_batch_persistent_supported": [pt(LstmSeq), _I, _I],
        "t2amd_lstm_seq_bwd2_batch_persistent_f32": [pt(LstmSeq), pt(LstmSeq), _P, _P, _P, _P],
        "t2amd_encoder_handoff_timeouts": [_I],
        "t2amd_decoder_infer_steps_f32": [pt(DecInfer), _P],
        "t2amd_struct_sizes": [pt(C.c_int), _I],
        "t2amd_set_validate_only": [_I],
        "t2amd_set_decoder_streams": [_I],
        "t2amd_set_bptt_cell_fold": [_I],
        "t2amd_get_bptt_cell_fold": [],
        "t2amd_set_small_batch_max": [_I],
        "t2amd_get_small_batch_max": [_I],
        "t2amd_dec_infer_uses_tiles": [_I, _I, _I, _I, _I, _I],
        "t2amd_attn_bwd_ws_floats": [_I, _I],
        "t2amd_set_attn_bwd_granules": [_I],
        "t2amd_attn_handoff_timeouts": [_I],
        "t2amd_set_attn_bwd_fused": [_I],
        "t2amd_attn_fwd_ws_floats": [_I, _I],
        "t2amd_set_attn_fwd_fused": [_I],
        "t2amd_lstm_step_small_f32": [pt(LstmStep), _P],
        "t2amd_linear_small_f32": [pt(SmallLinear), _P],
        "t2amd_profile_enable": [_I, _I],
        "t2amd_profile_read": [pt(C.c_float), pt(C.c_int)],
        "t2amd_profile_event_overhead": [pt(C.c_float)],
        "t2amd_reflect_pad_f32": [_P, _L, _P, _L, _I, _I, _I, _I, _P],
        "t2amd_stft_magnitude_f32": [_P, _L, _P, _L, _L, _I, _I, _P],
        "t2amd_mel_log_compress_f32": [_P, _L, _P, _I, _I, _I, _F, _P],
        "t2amd_mel_log_bwd_f32": [_P, _P, _L, _P, _L, _I, _I, _I, _F, _P],
        "t2amd_stft_magnitude_bwd_f32": [_P, _L, _P, _L, _P, _L, _L, _I, _I, _P],
        "t2amd_stft_frames_fold_f32": [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _I, _P],
        "t2amd_mel_l1_rows_per_slot": [_I],
        "t2amd_mel_l1_fwd_f32": [_P, _P, _P, _I, _I, _I, _I, _L, _P, _L, _P],
        "t2amd_mel_l1_bwd_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _L, _P, _P],
        "t2amd_stft_loss_rows_per_slot": [_I],
        "t2amd_stft_loss_fwd_f32": [_P, _L, _P, _L, _P, _I, _I, _I, _F, _P, _L, _P],
        "t2amd_stft_loss_finish_f64": [_P, _L, _P, _P, _I, _F, _F, _P, _P, _P, _P],
        "t2amd_stft_loss_bwd_f32": [_P, _L, _P, _L, _P, _P, _P, _I, _I, _I, _I, _F, _P, _L, _L, _P],
        "t2amd_stft_loss_sum_f32": [_P, _L, _L, _I, _L, _P, _P],
        "t2amd_resample_plan": [_I, _I, _I, _I, pt(C.c_int), pt(C.c_int)],
        "t2amd_resample_fwd_f32": [_P, _L, _P, _I, _L, _P, _L, _L, _P, _P, _I, _I, _I, _I, _P],
        "t2amd_resample_bwd_f32": [_P, _L, _P, _I, _L, _L, _P, _L, _P, _P, _I, _I, _I, _I, _I, _P],
        "t2amd_dtw_width": [],
        "t2amd_mel_cepstrum_f32": [_P, _L, _L, _P, _I, _I, _I, _P, _I, _P, _P],
        "t2amd_dtw_f32": [_P, _L, _P, _L, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P],
        "t2amd_dtw_backtrack": [_P, _I, _I, _P, _P, _P, _I, _I, _I, _P, _I, _P],
        "t2amd_yin_plan": [C.c_double, _I, _I, C.c_double, C.c_double, pt(C.c_int), pt(C.c_int)],
        "t2amd_yin_f32": [_P, _L, _P, _I, _L, _I, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P],
        "t2amd_align_limits": [pt(C.c_int), pt(C.c_int), pt(C.c_int)],
        "t2amd_align_workspace": [_I, _I, _I, pt(C.c_longlong)],
        "t2amd_monotonic_align_f32": [_P, _L, _L, _P, _P, _I, _I, _I, _P, _P, _P, _P, _L, _P],
        "t2amd_forward_sum_workspace": [_I, _I, _I, _I, pt(C.c_longlong)],
        "t2amd_forward_sum_f32": [_P, _L, _L, _P, _P, _I, _I, _I, _P, _I, _P, _L, _P],
        "t2amd_forward_sum_bwd_f32": [_P, _L, _L, _P, _P, _I, _I, _I, _P, _P, _P, _L, _L, _P, _P, _L, _P],
        "t2amd_aligner_workspace": [_I, _I, _I, _I, _I, pt(C.c_longlong)],
        "t2amd_aligner_pack_keys_f32": [_P, _P, _I, _I, _I, _P, _P, _P],
        "t2amd_aligner_transpose_f32": [_P, _P, _I, _I, _I, _P, _P],
        "t2amd_aligner_rows_fwd_f32": [_P, _L, _L, _P, _L, _L, _P, _P, _I, _I, _I, _P, _P],
        "t2amd_aligner_rows_bwd_f32": [_P, _L, _L, _P, _P, _I, _I, _I, _P, _P, _P, _P, _L, _L, _P],
        "t2amd_aligner_scores_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _L, _L, _P, _L, _L, _I, _P, _L, _P],
        "t2amd_aligner_scores_bwd_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _L, _L, _P, _P, _P, _L, _L, _P, _L, _P, _L, _P],
        "t2amd_aligner_product_f32": [_I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _L, _P, _L, _P],
        "t2amd_beta_binomial_log_prior_f32": [_P, _P, _I, _I, _I, C.c_double, _P, _P],
        "t2amd_regulate_limits": [pt(C.c_int), pt(C.c_int), pt(C.c_int)],
        "t2amd_durations_to_path_i32": [_P, _I, _L, _P, _I, _I, _I, _P, _P, _P, _P, _P],
        "t2amd_length_regulate_f32": [_P, _L, _L, _P, _I, _I, _I, _I, _P, _P],
        "t2amd_length_regulate_bwd_f32": [_P, _L, _L, _P, _I, _I, _I, _I, _P, _P],
        "t2amd_token_average_f32": [_P, _L, _L, _P, _L, _P, _I, _I, _I, _I, _P, _P, _P, _P],
        "t2amd_token_average_bwd_f32": [_P, _P, _P, _L, _P, _I, _I, _I, _I, _P, _P],
        "t2amd_self_attn_limits": [pt(C.c_int)] * 5,
        "t2amd_self_attn_workspace": [_I, _I, _I, _I, _I, pt(C.c_longlong)],
        "t2amd_self_attn_f32": [_P, _L, _L, _L] * 3 + [_P, _I, _I, _I, _I, _F, _P, _P, _P],
        "t2amd_self_attn_delta_f32": [_P, _L, _L, _L, _P, _P, _I, _I, _I, _I, _P, _P],
        "t2amd_self_attn_bwd_f32": [_P, _L, _L, _L] * 3 + [_P, _P, _P, _L, _L, _L, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _L, _P],
        "t2amd_fft_block_limits": [pt(C.c_int)] * 5,
        "t2amd_fft_block_workspace": [_I, _I, _I, _I, _I, _I, pt(C.c_longlong)],
        "t2amd_ffb_conv_f32": [_P, _L, _L, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
        "t2amd_ffb_conv_dw_f32": [_P, _P, _L, _L, _P, _I, _I, _I, _I, _I, _P, _P, _L, _P],
        "t2amd_ffb_transpose_f32": [_P, _P, _I, _I, _I, _P, _L, _P],
        "t2amd_ffb_dw_finish_f32": [_P, _I, _I, _I, _I, _P, _P],
        "t2amd_ffb_add_ln_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P],
        "t2amd_ffb_add_ln_bwd_f32": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P],
        "t2amd_ffb_colsum_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _L, _P],
        "t2amd_ffb_relu_mask_f32": [_P, _P, _P, _I, _I, _I, _P, _P],
        "t2amd_predictor_limits": [pt(C.c_int)] * 5,
        "t2amd_predictor_workspace": [_I, _I, _I, _I, _I, _I, pt(C.c_longlong)],
        "t2amd_pred_project_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
        "t2amd_pred_project_bwd_f32": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
        "t2amd_pred_project_sums_f32": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P],
        "t2amd_pred_embed_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
        "t2amd_pred_embed_bwd_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
        "t2amd_pred_embed_sums_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _L, _P],
        "t2amd_gl_overlap_add_f32": [_P, _L, _P, _P, _P, _I, _L, _I, _I, _F, _P, _L, _L, _I, _P],
        "t2amd_gl_project_f32": [_P, _L, _P, _L, _P, _P, _I, _L, _I, _I, _I, _I, _P, _L, _P],
        "t2amd_gl_rect_f32": [_P, _P, _L, _P, _P, _I, _L, _I, _I, _I, _I, _P, _L, _P, _L, _P],
        "t2amd_stft_polar_f32": [_P, _L, _I, _I, _I, _P, _P, _P],
        "t2amd_mel_decompress_f32": [_P, _I, _I, _I, _P, _P, _P, _L, _P],
        "t2amd_wg_layer_f32": [_P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P, _L, _P, _L, _I, _P, _L, _I, _P, _I, _P],
        "t2amd_wg_tail_f32": [_P, _L, _I, _P, _P, _I, _P, _P, _L, _P, _L, _L, _I, _F, _P, _P, _P, _L, _P, _L, _P, _P, _L,
                              _I, _P],
        "t2amd_wg_denoise_f32": [_P, _P, _I, _I, _L, _F, _P],
        "t2amd_wg_head_f32": [_P, _L, _I, _P, _P, _I, _P, _L, _L, _P, _L, _P, _L, _P, _L, _L, _I, _I, _P, _P, _P, _P, _L, _P,
                              _P, _L, _I, _I, _L, _P],
        "t2amd_wg_nll_chunk": [],
        "t2amd_wg_nll_f32": [_P, _L, _L, _I, _P, _L, _L, _I, _P, _I, _L, _P, _L, _P, _P],
        "t2amd_wg_layer_train_f32": [_P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P, _L, _P, _L, _I, _P, _L, _I, _P, _P, _L,
                                     _P, _L, _I, _P],
        "t2amd_wg_head_save_f32": [_P, _L, _I, _P, _P, _I, _P, _L, _L, _P, _L, _P, _L, _P, _L, _L, _I, _I, _P, _P, _P, _P, _L,
                                   _P, _P, _L, _I, _I, _L, _P, _L, _P],
        "t2amd_wg_head_bwd_rows": [],
        "t2amd_wg_head_bwd_f32": [_P, _L, _I, _P, _I, _P, _L, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _P, _I, _P, _L,
                                  _P, _L, _P, _P, _L, _I, _I, _L, _F, _F, _P],
        "t2amd_wg_partial_sum_f32": [_P, _L, _L, _P, _P],
        "t2amd_wg_gate_bwd_f32": [_P, _L, _P, _L, _P, _L, _I, _P, _L, _P, _L, _P],
        "t2amd_wg_weight_norm_short": [],
        "t2amd_wg_weight_norm_f32": [_P, _I, _L, _P, _P, _P, _P, _P],
        "t2amd_wg_weight_norm_bwd_f32": [_P, _I, _L, _P, _P, _P, _P, _P, _P, _F, _P],
        "t2amd_optim_chunk": [],
        "t2amd_grad_norm_f32": [pt(TensorList), _F, _P, _P, _P],
        "t2amd_adam_step_f32": [pt(TensorList), pt(AdamHyper), _P, _P],
        "t2amd_decoder_persist_mailbox_bytes": [_I, _I, _I, _I],
        "t2amd_decoder_persist_supported": [pt(DecPersist)],
        "t2amd_decoder_infer_persistent_f32": [pt(DecPersist), _P],
        "t2amd_loss_workspace_doubles": [],
        "t2amd_tacotron2_loss_fwd_f32": [_P, _P, _P, _L, _P, _P, _L, _P, _P, _P],
        "t2amd_tacotron2_loss_bwd_f32": [_P, _P, _P, _L, _P, _P, _L, _P, _P, _P, _P, _P],
        "t2amd_hg_conv_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _I, _I, _I, _I, _F, _P, _L, _L, _P, _L, _L, _F, _I, _P, _L, _I,
                              _I, _P],
        "t2amd_hg_upsample_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _I, _I, _I, _I, _F, _P, _L, _L, _P, _L, _I, _I, _P],
        "t2amd_hg_post_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _F, _P, _P, _L, _I, _P, _L, _L, _P],
        "t2amd_hg_pack_mel_f32": [_P, _L, _I, _I, _L, _P, _P, _L, _P, _I, _L, _P],
        "t2amd_vc_dwln_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _I, _P, _P, _F, _P, _L, _P, _L, _L, _P],
        "t2amd_vc_linear_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _I, _I, _P, _P, _L, _L, _P, _L, _L, _P, _L, _I, _P],
        "t2amd_vc_polar_f32": [_P, _L, _L, _L, _I, _F, _P, _L, _P, _L, _L, _P],
        "t2amd_vc_ola_f32": [_P, _L, _L, _L, _P, _P, _I, _I, _I, _I, _P, _L, _L, _P],
        "t2amd_vc_bwd_slot_rows": [],
        "t2amd_vc_ola_bwd_f32": [_P, _L, _L, _P, _P, _I, _P, _P, _L, _L, _I, _I, _I, _P, _L, _L, _P],
        "t2amd_vc_polar_bwd_f32": [_P, _L, _L, _L, _I, _F, _P, _L, _L, _P, _L, _P, _L, _L, _I, _P],
        "t2amd_vc_gelu_bwd_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _L, _L, _P],
        "t2amd_vc_gamma_bwd_f32": [_P, _L, _L, _L, _I, _P, _P, _L, _P, _L, _L, _P, _L, _P],
        "t2amd_vc_ln_bwd_f32": [_P, _L, _L, _L, _I, _P, _L, _P, _I, _P, _F, _P, _L, _P, _L, _L, _P, _L, _L, _P, _L, _P],
        "t2amd_vc_dw_bwd_f32": [_P, _L, _L, _L, _I, _P, _L, _L, _P, _L, _I, _P, _L, _P, _L, _L, _P, _L, _L, _P, _L, _P],
    }


_lib = None


class NativeError(RuntimeError):
    pass


def load():
    """dlopen the HIP library (once).  Raises NativeError when it is missing —
    there is no other compute path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "tacotron2_amd: %s not found. The MI355X engine has no fallback path; build it with "
            "`python -m tacotron2_amd.build` (needs hipcc)." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name in SYMBOLS:
        if not hasattr(lib, name):
            raise NativeError("tacotron2_amd: symbol %s missing from %s" % (name, LIB_PATH))
    for name, at in _argtypes().items():
        fn = getattr(lib, name)
        fn.argtypes = at
        fn.restype = C.c_int
    lib.t2amd_last_error.restype = C.c_char_p
    lib.t2amd_reflect_index.argtypes = [_L, _L]
    lib.t2amd_reflect_index.restype = C.c_longlong
    lib.t2amd_gl_packed_rows.argtypes = [_P, _I, _I, _I]
    lib.t2amd_gl_packed_rows.restype = C.c_longlong
    lib.t2amd_abi_version.restype = C.c_int
    lib.t2amd_attn_bwd_ws_floats.restype = C.c_longlong
    lib.t2amd_attn_fwd_ws_floats.restype = C.c_longlong
    lib.t2amd_decoder_persist_mailbox_bytes.restype = C.c_longlong
    lib.t2amd_lstm_seq_persistent_mailbox_bytes.restype = C.c_longlong
    lib.t2amd_lstm_seq_batch_persistent_flag_bytes.restype = C.c_longlong
    lib.t2amd_decoder_train_fwd_persistent_flag_bytes.restype = C.c_longlong
    if lib.t2amd_abi_version() != 1:
        raise NativeError("tacotron2_amd: ABI version mismatch")
    # the binary must be THESE sources' binary (by content: a snapshot copy or a checkout resets mtimes).  An explicitly
    # selected library (T2AMD_LIB: instrumented / A-B variants built by tacotron2_amd.build) carries the hash of the same
    # tree; T2AMD_ALLOW_STALE_LIB=1 is the escape hatch for a deliberately older binary.
    lib.t2amd_source_sha1.restype = C.c_char_p
    lib.t2amd_source_sha1.argtypes = []
    built = (lib.t2amd_source_sha1() or b"").decode()
    if os.path.isdir(os.path.join(_HERE, "csrc")) and os.environ.get("T2AMD_ALLOW_STALE_LIB", "0") != "1":
        from . import build as _build
        try:
            want = _build.source_sha1()
        except OSError as e:             # e.g. installed as package data without include/: nothing to compare against
            want = None
            if os.environ.get("T2AMD_REQUIRE_SOURCE_HASH", "0") == "1":
                raise NativeError("tacotron2_amd: cannot hash the kernel sources beside %s (%s)" % (LIB_PATH, e))
            # csrc/ is here but not everything the hash covers: say that the stale-library check did NOT happen --
            # silently loading whatever .so lies there would defeat "binary and sources are provably the same tree"
            import sys
            print("tacotron2_amd: warning: the kernel sources beside %s could not be hashed (%s); the library (built from %s) "
                  "is loaded WITHOUT the stale-library check (T2AMD_REQUIRE_SOURCE_HASH=1 makes this an error)"
                  % (LIB_PATH, e, built or "<unstamped sources>"), file=sys.stderr, flush=True)
        if want is not None and built != want:
            raise NativeError("tacotron2_amd: %s was built from other sources (binary %s, sources %s): run "
                              "`python -m tacotron2_amd.build` (or set T2AMD_ALLOW_STALE_LIB=1 to use it anyway)"
                              % (LIB_PATH, built or "<unstamped>", want))
    sizes = (C.c_int * 32)()
    n = lib.t2amd_struct_sizes(sizes, 32)
    if n != len(_STRUCTS):
        raise NativeError("tacotron2_amd: struct count mismatch (%d vs %d)" % (n, len(_STRUCTS)))
    for i, st in enumerate(_STRUCTS):
        if C.sizeof(st) != sizes[i]:
            raise NativeError("tacotron2_amd: sizeof(%s) = %d in Python, %d in the library"
                              % (st.__name__, C.sizeof(st), sizes[i]))
    _lib = lib
    return lib


def library_sha1():
    """Source hash compiled into the loaded library (``t2amd_source_sha1``)."""
    return (load().t2amd_source_sha1() or b"").decode()


_validate_only = False


def cast_bf16(src, dst):
    """dst (torch.bfloat16, contiguous) = bf16(src) with round-to-nearest-even."""
    _fullc(src), _fullc(dst)
    if src.numel() != dst.numel() or dst.dtype != torch.bfloat16:
        raise NativeError("cast_bf16: dst must be a bfloat16 tensor of the same size")
    _check(load().t2amd_cast_bf16_f32(ptr(src), ptr(dst, torch.bfloat16), src.numel(), _stream()), "t2amd_cast_bf16_f32")


def split_bf16x3(src, dst):
    """dst (torch.bfloat16, [rows][2 K], contiguous) = the split-bf16 operand image of src (f32 [rows][K], contiguous, K % 16 == 0):
    per 16 k, 16 hi = bf16(x) then 16 lo = bf16(x - hi) -- what t2amd_lstm_step.bf16 == 3 / the 'bf16x3' mode multiplies."""
    _fullc(src), _fullc(dst)
    K = src.shape[-1]
    rows = src.numel() // max(K, 1)
    if dst.dtype != torch.bfloat16 or dst.numel() != 2 * src.numel() or K % 16 != 0:
        raise NativeError("split_bf16x3: dst must be a bfloat16 tensor of twice the size, K %% 16 == 0 (src %s, dst %s)"
                          % (tuple(src.shape), tuple(dst.shape)))
    _check(load().t2amd_split_bf16x3_f32(ptr(src), _i64(K), ptr(dst, torch.bfloat16), _i64(K), _i64(rows), K, _stream()),
           "t2amd_split_bf16x3_f32")


def decoder_persist_mailbox_bytes(Ti, E, H, P):
    return int(load().t2amd_decoder_persist_mailbox_bytes(int(Ti), int(E), int(H), int(P)))


def decoder_persist_supported(desc):
    """None when the persistent single-utterance decode kernel can run this geometry, else the reason."""
    lib = load()
    if lib.t2amd_decoder_persist_supported(C.byref(desc)) == 0:
        return None
    msg = lib.t2amd_last_error()
    return msg.decode() if msg else "unsupported"


def decoder_infer_persistent(desc, reads=None, writes=None):
    """The whole free-running decode loop of ONE utterance as one persistent launch (csrc/decode_persist.hip)."""
    _loop("decoder_infer_persistent", "t2amd_decoder_infer_persistent_f32", [desc], reads, writes)


def tacotron2_loss_fwd(mel, post, tgt, gate, gate_tgt, ws, out4):
    for t in (mel, post, tgt, gate, gate_tgt, out4):
        _fullc(t)
    if mel.numel() != post.numel() or mel.numel() != tgt.numel() or gate.numel() != gate_tgt.numel():
        raise NativeError("tacotron2_loss: shape mismatch between outputs and targets")
    _check(load().t2amd_tacotron2_loss_fwd_f32(ptr(mel), ptr(post), ptr(tgt), mel.numel(), ptr(gate), ptr(gate_tgt),
                                               gate.numel(), ptr(ws, torch.float64), ptr(out4), _stream()),
           "t2amd_tacotron2_loss_fwd_f32")


def tacotron2_loss_bwd(mel, post, tgt, gate, gate_tgt, upstream, d_mel, d_post, d_gate):
    for t in (mel, post, tgt, gate, gate_tgt, upstream, d_mel, d_post, d_gate):
        _fullc(t)
    _check(load().t2amd_tacotron2_loss_bwd_f32(ptr(mel), ptr(post), ptr(tgt), mel.numel(), ptr(gate), ptr(gate_tgt),
                                               gate.numel(), ptr(upstream), ptr(d_mel), ptr(d_post), ptr(d_gate), _stream()),
           "t2amd_tacotron2_loss_bwd_f32")


def loss_workspace_doubles():
    return int(load().t2amd_loss_workspace_doubles())


_decoder_streams = 1


def set_decoder_streams(n):
    """1 (default): single stream, fused launches; 2: decoder-LSTM chain of the training loops on a side stream."""
    global _decoder_streams
    _check(load().t2amd_set_decoder_streams(int(n)), "t2amd_set_decoder_streams")
    _decoder_streams = int(n)


def decoder_streams():
    return _decoder_streams


def set_bptt_cell_fold(on):
    """1: the LSTM cell backwards of a decoder BPTT step run inside the step's attention-backward launch (5 dependent
    launches per time step instead of 6); 0: as a launch of their own.  Bit-identical gradients either way."""
    _check(load().t2amd_set_bptt_cell_fold(1 if on else 0), "t2amd_set_bptt_cell_fold")


def get_bptt_cell_fold():
    return int(load().t2amd_get_bptt_cell_fold())


def set_small_batch_max(n):
    """Free-running decoder: the largest batch the matrix-vector kernels serve (0 .. 8; -1 = by operand mode: 3 rows with bf16
    operands, 4 otherwise); above it the 64-row MFMA tiles."""
    _check(load().t2amd_set_small_batch_max(int(n)), "t2amd_set_small_batch_max")


def small_batch_max(bf16=0):
    """The boundary in force for operand mode ``bf16`` (t2amd_dec_infer.bf16: 0 f32, 1 bf16, 3 split-bf16)."""
    return int(load().t2amd_get_small_batch_max(int(bf16)))


def dec_infer_uses_tiles(B, bf16, E, Ha, Hd, P):
    """True when the free-running decoder's launch chain runs B rows in operand mode ``bf16`` on the 64-row tiles."""
    return bool(load().t2amd_dec_infer_uses_tiles(int(B), int(bf16), int(E), int(Ha), int(Hd), int(P)))


def small_batch_max_setting():
    """The raw setting (-1 = by operand mode), for save / restore around a test."""
    a, b = small_batch_max(0), small_batch_max(1)
    return -1 if a != b else a


def set_validate_only(on):
    """Argument-check mode for CPU tests: host logic runs, kernels are not launched, tensors may
    live on the CPU and outputs stay uninitialised.  Never a compute path."""
    global _validate_only
    load().t2amd_set_validate_only(1 if on else 0)
    _validate_only = bool(on)


def validate_only():
    return _validate_only


def profile_enable(tag, max_launches):
    """Bracket every LSTM-step launch with role `tag` (1 attention LSTM, 2 decoder LSTM) by HIP events."""
    _check(load().t2amd_profile_enable(tag, max_launches), "t2amd_profile_enable")


def profile_event_overhead():
    """ms of an empty event bracket on the launch stream (call before profile_read)."""
    ms = C.c_float(0)
    _check(load().t2amd_profile_event_overhead(C.byref(ms)), "t2amd_profile_event_overhead")
    return ms.value


def profile_read():
    """-> (total_ms, count) of the bracketed launches; disables profiling."""
    ms, n = C.c_float(0), C.c_int(0)
    _check(load().t2amd_profile_read(C.byref(ms), C.byref(n)), "t2amd_profile_read")
    return ms.value, n.value


def _check(rc, what):
    if rc != 0:
        msg = _lib.t2amd_last_error()
        raise NativeError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))


def _stream():
    if _validate_only:
        return None
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=torch.float32):
    """Raw device pointer of a tensor (None -> NULL), with dtype/device checks."""
    if t is None:
        return None
    if not t.is_cuda and not _validate_only:
        raise NativeError("tacotron2_amd: expected a device (HIP) tensor, got a %s tensor; the engine "
                          "has no CPU path" % t.device)
    if dtype is not None and t.dtype != dtype:
        raise NativeError("tacotron2_amd: expected %s, got %s" % (dtype, t.dtype))
    return C.c_void_p(t.data_ptr())


def _mat(t, dtype=torch.float32):
    """2-D view with unit inner stride -> (ptr, ld, rows, cols)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise NativeError("expected a 2-D tensor with contiguous rows, got shape %s stride %s"
                          % (tuple(t.shape), t.stride()))
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    return ptr(t, dtype), ld, t.shape[0], t.shape[1]


def _fullc(t):
    if not t.is_contiguous():
        raise NativeError("expected a contiguous tensor, got shape %s stride %s" % (tuple(t.shape), t.stride()))
    return t


def scale_for(p):
    """fp32 1/(1-p), formed like ATen's dropout (noise.div_(1-p))."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1.0 - p, dtype=torch.float32))


# ----------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------
def gemm_tile_size(M, N, precision, nz=1, a_km=False, b_kn=False):
    """Tile edge (128/256) the library will use for this product launched as nz = batch*splitk slices."""
    return int(load().t2amd_gemm_tile_size(int(M), int(N), int(precision), int(nz), 0 if a_km else 1, 0 if b_kn else 1))


def gemm(Cm, A, B, a_km=False, b_kn=False, accumulate=False, bias=None, act=0, keep=None,
         keep_scale=1.0, convA=None, convB=None, batch=1, strides=(0, 0, 0), splitk=1, partials=None,
         fast=False):
    """Cm[M,N] (+)= act(A.B + bias)*keep.

    A is a view [M,K] (default) or [K,M] when ``a_km``;  B is a view [N,K] (default, the
    nn.Linear weight layout) or [K,N] when ``b_kn``.  ``convA=(T,C,pad,sign)`` / ``convB=(T,C,pad)``
    switch on implicit-convolution addressing (see the header).  With ``splitk>1`` the partial
    results go to ``partials`` ([splitk, M*N] contiguous) and Cm is not written."""
    lib = load()
    d = GemmDesc()
    pa, lda, r0, c0 = _mat(A)
    pb, ldb, r1, c1 = _mat(B)
    pc, ldc, M, N = _mat(Cm)
    Ka, Ma = (r0, c0) if a_km else (c0, r0)
    Kb, Nb = (r1, c1) if b_kn else (c1, r1)
    if convA is not None:
        # A is the plain activation matrix [rows, C]; the virtual K is taps*C, taken from B
        if a_km or Ka != convA[1] or Kb % convA[1] != 0:
            raise NativeError("gemm: convA needs A=[rows,C] and K(B) a multiple of C")
        K = Kb
    else:
        K = Ka
    if convB is not None:
        # B is the plain activation matrix [rows, C] (K = rows); the virtual N is taps*C, taken from C
        if not b_kn or Nb != convB[1] or N % convB[1] != 0:
            raise NativeError("gemm: convB needs B=[rows,C] (b_kn) and N(C) a multiple of C")
        Nb = N
    if Ma != M or Nb != N or Kb != K:
        raise NativeError("gemm: shape mismatch C=%s A=%s B=%s (a_km=%s b_kn=%s K=%d)"
                          % (tuple(Cm.shape), tuple(A.shape), tuple(B.shape), a_km, b_kn, K))
    d.A, d.B, d.C = pa, pb, pc
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.a_kcontig = 0 if a_km else 1
    d.b_kcontig = 0 if b_kn else 1
    d.batch = batch
    d.strideA, d.strideB, d.strideC = strides
    d.splitk = splitk
    d.precision = int(fast)          # False/0 exact f32, True/1 split-bf16 x3, 2 plain bf16
    d.accumulate = 1 if accumulate else 0
    d.bias = ptr(bias)
    d.act = act
    if keep is not None:
        if keep.dim() != 2 or tuple(keep.shape) != (M, N) or keep.stride(1) != 1:
            raise NativeError("gemm: keep mask must be a [M,N] uint8 view, got %s" % (tuple(keep.shape),))
        d.keep, d.ldkeep, d.keep_scale = ptr(keep, torch.uint8), keep.stride(0), keep_scale
    if convA is not None:
        d.convA_T, d.convA_C, d.convA_pad, d.convA_sign = convA
    if convB is not None:
        d.convB_T, d.convB_C, d.convB_pad = convB
    if splitk > 1:
        if partials is None or partials.numel() < splitk * M * N or not partials.is_contiguous():
            raise NativeError("gemm: split-K needs a contiguous partials buffer")
        d.C = ptr(partials)
        d.ldc = N
        d.strideSplitC = M * N
    _check(lib.t2amd_gemm_f32(C.byref(d), _stream()), "t2amd_gemm_f32")


def gemm16_tn(Cm, A16, B16, K=None, splitk=1, partials=None, accumulate=False, bias=None):
    """Cm[M,N] (f32) = A16[M,K] . B16[N,K]^T, bf16 K-contiguous operands (csrc/gemm16.hip).  ``K`` defaults to the operands'
    width (a multiple of 64); with ``splitk`` > 1 the partial products go to ``partials`` (splitk, M*N)."""
    lib = load()
    d = Gemm16Desc()
    pa, lda, M, Ka = _mat(A16, torch.bfloat16)
    pb, ldb, N, Kb = _mat(B16, torch.bfloat16)
    K = Ka if K is None else K
    if K > Ka or K > Kb or Cm.shape[0] != M or Cm.shape[1] != N:
        raise NativeError("gemm16_tn: shape mismatch A=%s B=%s C=%s K=%d" % (tuple(A16.shape), tuple(B16.shape), tuple(Cm.shape), K))
    d.A, d.B, d.M, d.N, d.K, d.lda, d.ldb = pa, pb, M, N, K, lda, ldb
    d.splitk = splitk
    if splitk > 1:
        if partials is None or partials.numel() < splitk * M * N:
            raise NativeError("gemm16_tn: split-K needs a (splitk, M*N) partials buffer")
        d.C, d.ldc, d.strideSplitC = ptr(partials), N, M * N
    else:
        d.C, d.ldc = _mat(Cm)[:2]
    d.accumulate = 1 if accumulate else 0
    d.bias = ptr(bias)
    _check(lib.t2amd_gemm16_tn(C.byref(d), _stream()), "t2amd_gemm16_tn")


def conv16(Cm, img16, W16, B, T, pad, bias=None, accumulate=False):
    """1-d convolution over channel-last rows on the bf16-resident product: Cm[(b T + t), co] (+)= sum_{tap, ci}
    img16[b (T + 2 pad) + t + tap][ci] * W16[co][tap Ci + ci] (+ bias).  ``img16`` is cast_halo_bf16's image
    ((B (T + 2 pad) + 2 pad) rows of Ci), ``W16`` the bf16 weights packed [Co][k Ci]."""
    lib = load()
    d = Gemm16Desc()
    Ci = img16.shape[1]
    Tp = T + 2 * pad
    pw, ldw, Co, K = _mat(W16, torch.bfloat16)
    # K may be the window length k Ci rounded up to the 64-deep k-steps (zero weight columns, pack_conv_bf16): the overhang of
    # the last real window, row (B - 1) Tp + T - 1, must stay inside the image's trailing 2 pad halo rows
    klen = (2 * pad + 1) * Ci
    if img16.shape[0] < B * Tp + 2 * pad or K < klen or K - klen > 2 * pad * Ci or Cm.shape[0] != B * T or Cm.shape[1] != Co:
        raise NativeError("conv16: shape mismatch img=%s W=%s C=%s" % (tuple(img16.shape), tuple(W16.shape), tuple(Cm.shape)))
    d.A, d.lda = ptr(_fullc(img16), torch.bfloat16), Ci
    d.B, d.ldb = pw, ldw
    d.C, d.ldc = _mat(Cm)[:2]
    d.M, d.N, d.K = (B - 1) * Tp + T, Co, K             # window rows up to the last real output (the rest would be discarded)
    d.splitk, d.accumulate, d.bias = 1, 1 if accumulate else 0, ptr(bias)
    d.win_T, d.win_Tp = T, Tp
    _check(lib.t2amd_gemm16_tn(C.byref(d), _stream()), "t2amd_gemm16_tn")


def _kk_desc(Cm, A16, B16, K, M=None, N=None, lda=None, ldb=None, splitk=1, partials=None, accumulate=False, bias=None):
    d = Gemm16Desc()
    pa, lda0, ra, wa = _mat(A16, torch.bfloat16)
    pb, ldb0, rb, wb = _mat(B16, torch.bfloat16)
    M = wa if M is None else M
    N = wb if N is None else N
    lda = lda0 if lda is None else lda
    ldb = ldb0 if ldb is None else ldb
    # the elements a product touches must lie inside the tensors handed in (contiguous storage from their first element)
    span_a = (ra - 1) * lda0 + wa
    span_b = (rb - 1) * ldb0 + wb
    if K < 1 or (K - 1) * lda + M > span_a or (K - 1) * ldb + N > span_b or Cm.shape[0] != M or Cm.shape[1] != N:
        raise NativeError("gemm16_kk: shape mismatch A=%s B=%s C=%s M=%d N=%d K=%d lda=%d ldb=%d"
                          % (tuple(A16.shape), tuple(B16.shape), tuple(Cm.shape), M, N, K, lda, ldb))
    d.A, d.B, d.M, d.N, d.K, d.lda, d.ldb = pa, pb, M, N, K, lda, ldb
    d.splitk = splitk
    if splitk > 1:
        if partials is None or partials.numel() < splitk * M * N:
            raise NativeError("gemm16_kk: split-K needs a (splitk, M*N) partials buffer")
        d.C, d.ldc, d.strideSplitC = ptr(partials), N, M * N
    else:
        d.C, d.ldc = _mat(Cm)[:2]
    d.accumulate = 1 if accumulate else 0
    d.bias = ptr(bias)
    return d


def gemm16_kk(Cm, A16, B16, K, M=None, N=None, lda=None, ldb=None, splitk=1, partials=None, accumulate=False, bias=None):
    """Cm[M,N] (f32) = sum_k A16[k, m] . B16[k, n]: bf16 K-MAJOR operands (csrc/gemm16.hip, transposing LDS reads) -- the
    layout of the time loops' slabs and of channel-last images.  ``A16`` / ``B16`` are 2-D bf16 tensors whose rows are the k
    index; ``M`` / ``N`` / ``lda`` / ``ldb`` default to their widths and row strides.  A row stride SMALLER than the width
    expresses overlapping rows (B[k][n] = img[k Ci + n], n < taps Ci: the windows of a convolution); the tensor must then
    hold the last row's reach.  With ``splitk`` > 1 the partial products go to ``partials`` (splitk, M*N)."""
    d = _kk_desc(Cm, A16, B16, K, M, N, lda, ldb, splitk, partials, accumulate, bias)
    _check(load().t2amd_gemm16_kk(C.byref(d), _stream()), "t2amd_gemm16_kk")


def gemm16_kk_group(problems):
    """Up to four K-major products in one launch (same M, same splitk): ``problems`` is a list of keyword dictionaries of
    gemm16_kk.  Their workgroups run side by side on the same rows of A (read once): the input blocks of an LSTM's dW."""
    if not 1 <= len(problems) <= 4:
        raise NativeError("gemm16_kk_group: 1..4 problems, got %d" % len(problems))
    arr = (Gemm16Desc * len(problems))(*[_kk_desc(**kw) for kw in problems])
    # through the dispatcher when the registration library is there (torch.ops.tacotron2_amd.wgrad_gemm16), else ctypes
    reads = [kw[k_] for kw in problems for k_ in ('A16', 'B16')]
    writes = [kw['partials'] if kw.get('partials') is not None else kw['Cm'] for kw in problems]
    if not _via_ops("wgrad_gemm16", [arr], reads, writes):
        _check(load().t2amd_gemm16_kk_group(arr, len(problems), _stream()), "t2amd_gemm16_kk_group")


def pack_conv_bf16(W, reversed=False):
    """bf16 image of a Conv1d weight (Co, Ci, k) for the window mode: [Co][Kp] rows (tap, ci) for the forward, or, with
    ``reversed``, [Ci][Kp] rows (k - 1 - tap, co) for the data gradient; Kp = the row length rounded up to 64, zero behind it."""
    Co, Ci, k = W.shape
    rows, inner = (Ci, Co) if reversed else (Co, Ci)
    Kp = (k * inner + 63) // 64 * 64
    out = torch.empty(rows, Kp, dtype=torch.bfloat16, device=W.device)
    _check(load().t2amd_pack_conv_bf16(ptr(_fullc(W)), ptr(out, torch.bfloat16), Co, Ci, k, Kp, 1 if reversed else 0, _stream()),
           "t2amd_pack_conv_bf16")
    return out


def cast_halo_bf16(src, dst, T, pad):
    """dst[(b (T + 2 pad) + pad + t), c] (bf16) = src[(b T + t), c]; every row of the image -- (rows / T) (T + 2 pad) + 2 pad of
    them -- is written, the halo rows with zeros (dst need not be initialised)."""
    ps, lds, rows, Cc = _mat(src)
    if dst.dtype != torch.bfloat16 or dst.shape[1] != Cc or dst.shape[0] < (rows // T) * (T + 2 * pad) + 2 * pad:
        raise NativeError("cast_halo_bf16: shape mismatch src=%s dst=%s" % (tuple(src.shape), tuple(dst.shape)))
    _check(load().t2amd_cast_halo_bf16(ps, _i64(lds), ptr(_fullc(dst), torch.bfloat16), _i64(rows), Cc, T, pad, _stream()),
           "t2amd_cast_halo_bf16")


def transpose_cast_bf16(src, dst, rows_padded=None):
    """dst[c, r] (bf16) = src[r, c] (f32 or bf16); columns rows..rows_padded-1 of dst are zeroed."""
    lib = load()
    is16 = src.dtype == torch.bfloat16
    ps, lds, rows, cols = _mat(src, torch.bfloat16 if is16 else torch.float32)
    pd, ldd, c2, rp = _mat(dst, torch.bfloat16)
    rows_padded = rp if rows_padded is None else rows_padded
    if c2 != cols or rows_padded < rows or rows_padded > rp:
        raise NativeError("transpose_cast_bf16: shape mismatch src=%s dst=%s" % (tuple(src.shape), tuple(dst.shape)))
    _check(lib.t2amd_transpose_cast_bf16(ps, 1 if is16 else 0, _i64(lds), pd, _i64(ldd), rows, cols, rows_padded, _stream()),
           "t2amd_transpose_cast_bf16")


def splitk_reduce(partials, nsplit, out, accumulate=False, perm_taps=0, perm_ci=0):
    lib = load()
    n = out.numel()
    _fullc(out)
    _check(lib.t2amd_splitk_reduce_f32(ptr(partials), nsplit, _i64(n), ptr(out), _i64(n),
                                       1 if accumulate else 0, perm_taps, perm_ci, _stream()),
           "t2amd_splitk_reduce_f32")


def splitk_reduce2d(partials, nsplit, out, accumulate=False):
    """out[r, c] (+)= sum_s partials[s][r cols + c]; ``out`` may be a column block of a wider matrix."""
    po, ldo, rows, cols = _mat(out)
    _check(load().t2amd_splitk_reduce2d_f32(ptr(partials), nsplit, _i64(rows * cols), po, rows, cols, _i64(ldo),
                                            1 if accumulate else 0, _stream()), "t2amd_splitk_reduce2d_f32")


# ----------------------------------------------------------------------------
# normalisation / elementwise
# ----------------------------------------------------------------------------
def bn_stats(x, ws, mean, invstd, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    lib = load()
    px, ldx, M, N = _mat(x)
    _check(lib.t2amd_bn_stats_f32(px, _i64(ldx), M, N, ptr(ws, torch.float64), ptr(mean), ptr(invstd),
                                  ptr(running_mean), ptr(running_var), C.c_float(momentum), C.c_float(eps),
                                  _stream()), "t2amd_bn_stats_f32")


def bn_eval_invstd(running_var, invstd, eps=1e-5):
    lib = load()
    _check(lib.t2amd_bn_eval_invstd_f32(ptr(running_var), ptr(invstd), running_var.numel(), C.c_float(eps),
                                        _stream()), "t2amd_bn_eval_invstd_f32")


def bn_act_fwd(x, y, mean, invstd, gamma, beta, act, keep=None, keep_scale=1.0, lens=None, T=0):
    lib = load()
    px, ldx, M, N = _mat(x)
    py, ldy, M2, N2 = _mat(y)
    assert (M, N) == (M2, N2)
    pk, ldk = (None, 0)
    if keep is not None:
        assert tuple(keep.shape) == (M, N) and keep.stride(1) == 1
        pk, ldk = ptr(keep, torch.uint8), keep.stride(0)
    _check(lib.t2amd_bn_act_fwd_f32(px, _i64(ldx), py, _i64(ldy), M, N, ptr(mean), ptr(invstd), ptr(gamma),
                                    ptr(beta), act, pk, _i64(ldk), C.c_float(keep_scale),
                                    ptr(lens, torch.int32), T, _stream()), "t2amd_bn_act_fwd_f32")


def bn_act_fwd_img(x, y, mean, invstd, gamma, beta, act, keep, keep_scale, y_img, T, pad):
    """bn_act_fwd with y leaving also as the bf16 halo image ``y_img`` ([M/T (T + 2 pad) + 2 pad][N]) the next convolution reads."""
    lib = load()
    px, ldx, M, N = _mat(x)
    py, ldy, M2, N2 = _mat(y)
    assert (M, N) == (M2, N2)
    pk, ldk = (None, 0)
    if keep is not None:
        assert tuple(keep.shape) == (M, N) and keep.stride(1) == 1
        pk, ldk = ptr(keep, torch.uint8), keep.stride(0)
    assert y_img.is_contiguous() and y_img.dtype == torch.bfloat16 and tuple(y_img.shape) == ((M // T) * (T + 2 * pad) + 2 * pad, N)
    _check(lib.t2amd_bn_act_fwd_img_f32(px, _i64(ldx), py, _i64(ldy), M, N, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), act, pk,
                                        _i64(ldk), C.c_float(keep_scale), ptr(y_img, torch.bfloat16), int(T), int(pad), _stream()),
           "t2amd_bn_act_fwd_img_f32")


def bn_act_bwd(dy, y, x, mean, invstd, gamma, act, keep, keep_scale, ws, dgamma, dbeta):
    lib = load()
    pd, ldd, M, N = _mat(dy)
    py, ldy, _, _ = _mat(y)
    px, ldx, _, _ = _mat(x)
    pk, ldk = (None, 0)
    if keep is not None:
        assert tuple(keep.shape) == (M, N) and keep.stride(1) == 1
        pk, ldk = ptr(keep, torch.uint8), keep.stride(0)
    _check(lib.t2amd_bn_act_bwd_f32(pd, _i64(ldd), py, _i64(ldy), px, _i64(ldx), M, N, ptr(mean), ptr(invstd),
                                    ptr(gamma), act, pk, _i64(ldk), C.c_float(keep_scale),
                                    ptr(ws, torch.float64), ptr(dgamma), ptr(dbeta), _stream()),
           "t2amd_bn_act_bwd_f32")


def bn_act_bwd_img(dy, y, x, mean, invstd, gamma, act, keep, keep_scale, ws, dgamma, dbeta, dx_img, T, pad, dbias, keep_f32=False):
    """bn_act_bwd with stage 2's output leaving as the bf16 halo image ``dx_img`` ([M/T (T + 2 pad) + 2 pad][N]) and as the bias
    gradient ``dbias`` [N] (t2amd_bn_act_bwd_img_f32); ``keep_f32``: also as the f32 slab in ``dy``."""
    lib = load()
    pd, ldd, M, N = _mat(dy)
    py, ldy, _, _ = _mat(y)
    px, ldx, _, _ = _mat(x)
    pk, ldk = (None, 0)
    if keep is not None:
        assert tuple(keep.shape) == (M, N) and keep.stride(1) == 1
        pk, ldk = ptr(keep, torch.uint8), keep.stride(0)
    assert dx_img.is_contiguous() and dx_img.dtype == torch.bfloat16 and tuple(dx_img.shape) == ((M // T) * (T + 2 * pad) + 2 * pad, N)
    assert dbias.numel() == N
    _check(lib.t2amd_bn_act_bwd_img_f32(pd, _i64(ldd), py, _i64(ldy), px, _i64(ldx), M, N, ptr(mean), ptr(invstd),
                                        ptr(gamma), act, pk, _i64(ldk), C.c_float(keep_scale),
                                        ptr(ws, torch.float64), ptr(dgamma), ptr(dbeta), ptr(dx_img, torch.bfloat16), int(T), int(pad),
                                        ptr(dbias), 1 if keep_f32 else 0, _stream()),
           "t2amd_bn_act_bwd_img_f32")


def colsum(x, ws, out, accumulate=False):
    lib = load()
    px, ldx, M, N = _mat(x)
    assert out.numel() == N
    _check(lib.t2amd_colsum_f32(px, _i64(ldx), M, N, ptr(ws, torch.float64), ptr(out), 1 if accumulate else 0,
                                _stream()), "t2amd_colsum_f32")


def colsum16(x16, ws, out, accumulate=False):
    """Column sums of a bf16 slab [M][N] (row stride in elements) into f32 ``out`` [N]."""
    lib = load()
    assert x16.dtype == torch.bfloat16 and x16.dim() == 2 and x16.stride(1) == 1 and out.numel() == x16.shape[1]
    _check(lib.t2amd_colsum_bf16(ptr(x16, torch.bfloat16), _i64(x16.stride(0)), x16.shape[0], x16.shape[1], ptr(ws, torch.float64),
                                 ptr(out), 1 if accumulate else 0, _stream()), "t2amd_colsum_bf16")


def embedding_fwd(ids, table, out):
    lib = load()
    rows = ids.numel()
    _check(lib.t2amd_embedding_fwd_f32(ptr(_fullc(ids), torch.int64), ptr(_fullc(table)), ptr(_fullc(out)),
                                       _i64(rows), table.shape[1], table.shape[0], _stream()),
           "t2amd_embedding_fwd_f32")


def embedding_bwd(ids, dout, dtable, ws=None):
    lib = load()
    rows = ids.numel()
    _check(lib.t2amd_embedding_bwd_f32(ptr(_fullc(ids), torch.int64), ptr(_fullc(dout)), ptr(_fullc(dtable)),
                                       None, _i64(rows), dtable.shape[1], dtable.shape[0], _stream()),
           "t2amd_embedding_bwd_f32")


def philox_keep_mask(out, p, seed, offset=0):
    lib = load()
    _check(lib.t2amd_philox_keep_mask(ptr(_fullc(out), torch.uint8), _i64(out.numel()), C.c_float(p),
                                      C.c_ulonglong(seed), C.c_ulonglong(offset), _stream()),
           "t2amd_philox_keep_mask")


def fill(t, v):
    lib = load()
    _check(lib.t2amd_fill_f32(ptr(_fullc(t)), _i64(t.numel()), C.c_float(v), _stream()), "t2amd_fill_f32")


def copy2d(dst, src, src2=None):
    lib = load()
    pd, ldd, R, Cc = _mat(dst)
    ps, lds, R1, C1 = _mat(src)
    assert (R, Cc) == (R1, C1), (dst.shape, src.shape)
    p2, ld2 = (None, 0)
    if src2 is not None:
        p2, ld2, R2, C2 = _mat(src2)
        assert (R, Cc) == (R2, C2)
    _check(lib.t2amd_copy2d_f32(ps, _i64(lds), p2, _i64(ld2), pd, _i64(ldd), R, Cc, _stream()), "t2amd_copy2d_f32")


def transpose(dst, src, batch=1, sstride=0, dstride=0):
    """dst[c][r] = src[r][c] for 2-D views (per batch item)."""
    lib = load()
    ps, lds, R, Cc = _mat(src)
    pd, ldd, R1, C1 = _mat(dst)
    assert (R1, C1) == (Cc, R), (dst.shape, src.shape)
    _check(lib.t2amd_transpose_f32(ps, _i64(lds), pd, _i64(ldd), R, Cc, batch, _i64(sstride), _i64(dstride),
                                   _stream()), "t2amd_transpose_f32")


def frames_to_time_major(mels, x0):
    lib = load()
    B, Cm, To = mels.shape
    assert tuple(x0.shape) == (To, B, Cm)
    _check(lib.t2amd_frames_to_time_major_f32(ptr(_fullc(mels)), ptr(_fullc(x0)), B, Cm, To, _stream()),
           "t2amd_frames_to_time_major_f32")


def split_projection(pg, mel_cl, gate, out_lens):
    lib = load()
    B, To, Cm = mel_cl.shape
    assert pg.numel() == To * B * (Cm + 1)
    _check(lib.t2amd_split_projection_f32(ptr(_fullc(pg)), ptr(_fullc(mel_cl)), ptr(_fullc(gate)),
                                          ptr(out_lens, torch.int32), B, Cm, To, _stream()),
           "t2amd_split_projection_f32")


def finalize_outputs(mel_cl, post_cl, mel, mel_post, out_lens):
    lib = load()
    B, To, Cm = mel_cl.shape
    _check(lib.t2amd_finalize_outputs_f32(ptr(_fullc(mel_cl)), ptr(post_cl), ptr(_fullc(mel)), ptr(mel_post),
                                          ptr(out_lens, torch.int32), B, Cm, To, _stream()),
           "t2amd_finalize_outputs_f32")


def grads_to_channel_last(dmel, dmel_post, dmel_cl, dpost_cl):
    lib = load()
    B, To, Cm = dmel_cl.shape
    _check(lib.t2amd_grads_to_channel_last_f32(ptr(dmel), ptr(dmel_post), ptr(_fullc(dmel_cl)),
                                               ptr(_fullc(dpost_cl)), B, Cm, To, _stream()),
           "t2amd_grads_to_channel_last_f32")


def gather_dout(dmel_cl, dgate, dout):
    lib = load()
    B, To, Cm = dmel_cl.shape
    _check(lib.t2amd_gather_dout_f32(ptr(_fullc(dmel_cl)), ptr(dgate), ptr(_fullc(dout)), B, Cm, To, _stream()),
           "t2amd_gather_dout_f32")


def relu_dropout_bwd(dy, y, scale):
    lib = load()
    assert dy.shape == y.shape
    _check(lib.t2amd_relu_dropout_bwd_f32(ptr(_fullc(dy)), ptr(_fullc(y)), C.c_float(scale), _i64(dy.numel()),
                                          _stream()), "t2amd_relu_dropout_bwd_f32")


# ----------------------------------------------------------------------------
# recurrent / attention single steps (used by the unit tests; the loops call them in C)
# ----------------------------------------------------------------------------
def _seg(t, width, dtype=torch.float32, x3=False):
    """``x3``: t is a split-bf16 image (split_bf16x3: 2 bf16 per k); width and ld count k, as for f32."""
    s = Seg()
    if t is None:
        s.p, s.ld, s.width = None, width, width
    else:
        p, ld, _, cols = _mat(t, dtype)
        if x3:
            if cols != 2 * width or ld % 2:
                raise NativeError("split-bf16 segment: expected %d columns (2 per k), got %d (ld %d)" % (2 * width, cols, ld))
            ld //= 2
        else:
            assert cols == width
        s.p, s.ld, s.width = p, ld, width
    return s


def lstm_step_fwd(xs, widths, W, H, B, gates_out, c_out, h_out, gin=None, bias=None, c_prev=None,
                  keep=None, keep_scale=1.0, lens=None, t=0, small=False, bf16=False, h16_out=None):
    """``bf16=True``: xs and W are torch.bfloat16 (MFMA operands), everything else stays f32.  ``bf16=3``: xs, W and h16_out are
    split-bf16 images (split_bf16x3: bfloat16 tensors with two columns per k) -- the 'bf16x3' mode of the wide tile.
    ``bf16=2`` (``small=True`` only): W alone is torch.bfloat16, xs stay f32 -- the decode loops' bf16-weight matrix-vector form.
    ``gates_out=None``: the gates are not written."""
    lib = load()
    a = LstmStep()
    a.nseg = len(xs)
    x3 = bf16 == 3 and bf16 is not True
    w_only = bf16 == 2 and bf16 is not True
    odt = torch.bfloat16 if bf16 and not w_only else torch.float32
    for i, (x, w) in enumerate(zip(xs, widths)):
        a.x[i] = _seg(x, w, odt, x3)
    a.W = ptr(_fullc(W), torch.bfloat16 if bf16 else torch.float32)
    a.bf16 = 3 if x3 else 2 if w_only else (1 if bf16 else 0)
    if h16_out is not None:
        a.h16_out, a.ld_h16 = _mat(h16_out, torch.bfloat16)[:2]
        if x3:
            a.ld_h16 //= 2
    a.Ktot, a.H, a.B = sum(widths), H, B
    if gin is not None:
        a.gin, a.ld_gin = _mat(gin)[:2]
    a.bias = ptr(bias)
    if c_prev is not None:
        a.c_prev, a.ld_cprev = _mat(c_prev)[:2]
    if gates_out is not None:
        a.gates_out, a.ld_gates = _mat(gates_out)[:2]
    a.c_out, a.ld_c = _mat(c_out)[:2]
    a.h_out, a.ld_h = _mat(h_out)[:2]
    if keep is not None:
        a.keep, a.ld_keep, a.keep_scale = ptr(keep, torch.uint8), keep.stride(0), keep_scale
    a.lens = ptr(lens, torch.int32)
    a.t = t
    if small:
        _check(lib.t2amd_lstm_step_small_f32(C.byref(a), _stream()), "t2amd_lstm_step_small_f32")
    else:
        _check(lib.t2amd_lstm_step_fwd_f32(C.byref(a), _stream()), "t2amd_lstm_step_fwd_f32")


def linear_small(X, W, Y, bias=None, act=0, keep=None, keep_scale=1.0):
    """Y[B,N] = act(X[B,K] . W[N,K]^T + bias) * keep, B <= 8 (matrix-vector kernel)."""
    lib = load()
    a = SmallLinear()
    a.X, a.ldx, Bx, K = _mat(X)
    a.W, a.ldw, N, Kw = _mat(W)
    a.Y, a.ldy, By, Ny = _mat(Y)
    if K != Kw or N != Ny or Bx != By:
        raise NativeError("linear_small: shape mismatch")
    a.B, a.N, a.K, a.act = Bx, N, K, act
    a.bias = ptr(bias)
    if keep is not None:
        a.keep, a.ldkeep, a.keep_scale = ptr(keep, torch.uint8), keep.stride(0), keep_scale
    _check(lib.t2amd_linear_small_f32(C.byref(a), _stream()), "t2amd_linear_small_f32")


def skinny_gemm(xs, widths, W, N, B, Y, nsplit=1, bf16=False, bias=None, act=0, keep=None, keep_scale=1.0):
    """Y[nsplit, B, N] = [xs...] . W[N, K]^T   (``bf16=3``: xs and W are split-bf16 images, see lstm_step_fwd)"""
    lib = load()
    a = SkinnyGemm()
    a.nseg = len(xs)
    x3 = bf16 == 3 and bf16 is not True
    odt = torch.bfloat16 if bf16 else torch.float32
    for i, (x, w) in enumerate(zip(xs, widths)):
        a.x[i] = _seg(x, w, odt, x3)
    a.W = ptr(_fullc(W), odt)
    a.bf16 = 3 if x3 else (1 if bf16 else 0)
    a.Ktot, a.N, a.B = sum(widths), N, B
    _fullc(Y)
    a.Y, a.ldy, a.nsplit, a.split_stride = ptr(Y), N, nsplit, B * N
    if bias is not None:
        a.bias = ptr(_fullc(bias))
    a.act = int(act)
    if keep is not None:
        a.keep, a.ld_keep, a.keep_scale = ptr(_fullc(keep), torch.uint8), keep.stride(0), keep_scale
    _check(lib.t2amd_skinny_gemm_f32(C.byref(a), _stream()), "t2amd_skinny_gemm_f32")


def _addend(t, nsplit=1, split_stride=0):
    a = Addend()
    if t is None:
        a.p, a.ld, a.nsplit, a.split_stride = None, 0, 1, 0
    else:
        p, ld, _, _ = _mat(t)
        a.p, a.ld, a.nsplit, a.split_stride = p, ld, nsplit, split_stride
    return a


def lstm_bwd_desc(B, H, dh_list, gates, c_prev, c, keep, keep_scale, dc, dgates, lens=None, t=0, dgates16=None, x3=False):
    """One cell-backward descriptor.  dh_list entries: a tensor, None, or (tensor, nsplit, split_stride) for an addend
    made of partial slabs."""
    a = LstmBwd()
    a.B, a.H = B, H
    for i in range(3):
        d = dh_list[i] if i < len(dh_list) else None
        a.dh[i] = _addend(*d) if isinstance(d, tuple) else _addend(d)
    a.gates, a.ld_gates = _mat(gates)[:2]
    if c_prev is not None:
        a.c_prev, a.ld_cprev = _mat(c_prev)[:2]
    a.c, a.ld_c = _mat(c)[:2]
    if keep is not None:
        a.keep, a.ld_keep, a.keep_scale = ptr(keep, torch.uint8), keep.stride(0), keep_scale
    a.dc, a.ld_dc = _mat(dc)[:2]
    a.dgates, a.ld_dgates = _mat(dgates)[:2]
    a.lens = ptr(lens, torch.int32)
    a.t = t
    if dgates16 is not None:
        a.dgates16, a.ld_dgates16 = ptr(dgates16, torch.bfloat16), dgates16.stride(0)
        if x3:                           # split-bf16 image of the gate gradients: [B][2 * 4H] bf16, ld in k
            a.ld_dgates16, a.dgates16_x3 = dgates16.stride(0) // 2, 1
    return a


def lstm_pointwise_bwd2(a, b=None):
    """The stand-alone launch for one or two descriptors of lstm_bwd_desc()."""
    _check(load().t2amd_lstm_pointwise_bwd2_f32(C.byref(a), C.byref(b) if b is not None else None, _stream()),
           "t2amd_lstm_pointwise_bwd2_f32")


def lstm_pointwise_bwd(B, H, dh_list, gates, c_prev, c, keep, keep_scale, dc, dgates, lens=None, t=0):
    lib = load()
    a = LstmBwd()
    a.B, a.H = B, H
    for i in range(3):
        a.dh[i] = _addend(dh_list[i] if i < len(dh_list) else None)
    a.gates, a.ld_gates = _mat(gates)[:2]
    if c_prev is not None:
        a.c_prev, a.ld_cprev = _mat(c_prev)[:2]
    a.c, a.ld_c = _mat(c)[:2]
    if keep is not None:
        a.keep, a.ld_keep, a.keep_scale = ptr(keep, torch.uint8), keep.stride(0), keep_scale
    a.dc, a.ld_dc = _mat(dc)[:2]
    a.dgates, a.ld_dgates = _mat(dgates)[:2]
    a.lens = ptr(lens, torch.int32)
    a.t = t
    _check(lib.t2amd_lstm_pointwise_bwd_f32(C.byref(a), _stream()), "t2amd_lstm_pointwise_bwd_f32")


def fold_location(wdense, wconv, U):
    """U buffer: 128*62 floats."""
    lib = load()
    assert U.numel() == ATT_DIM * LOC_TAPS
    assert tuple(wdense.shape) == (ATT_DIM, LOC_FILTERS) and tuple(wconv.shape) == (LOC_FILTERS, 2, LOC_KERNEL)
    _check(lib.t2amd_fold_location_f32(ptr(_fullc(wdense)), ptr(_fullc(wconv)), ptr(_fullc(U)), _stream()),
           "t2amd_fold_location_f32")


def unfold_location_grads(dU_acc, dv_acc, nb, wdense, wconv, dwdense, dwconv, dv):
    lib = load()
    _check(lib.t2amd_unfold_location_grads_f32(ptr(_fullc(dU_acc)), ptr(_fullc(dv_acc)), nb, ptr(_fullc(wdense)),
                                               ptr(_fullc(wconv)), ptr(_fullc(dwdense)), ptr(_fullc(dwconv)),
                                               ptr(_fullc(dv)), _stream()), "t2amd_unfold_location_grads_f32")


def attn_fwd_ws_floats(B, Ti):
    """partial energies + the granule block of the one-launch form (t2amd_attn_fwd_ws_floats; a multiple of 4)."""
    return int(load().t2amd_attn_fwd_ws_floats(int(B), int(Ti)))


_attn_fused_sel = {"fwd": -1, "bwd": -1}     # what this process last selected (-1: the library's default / environment)


def set_attn_fwd_fused(on):
    """K_e and K_c of an attention step as one launch (1), two launches (0), or the library default (-1)."""
    _check(load().t2amd_set_attn_fwd_fused(int(on)), "t2amd_set_attn_fwd_fused")
    _attn_fused_sel["fwd"] = int(on)


def get_attn_fwd_fused():
    """The last selection made through set_attn_fwd_fused (-1: none; the library default)."""
    return _attn_fused_sel["fwd"]


def get_attn_bwd_fused():
    return _attn_fused_sel["bwd"]


def attn_bwd_ws_floats(B, Ti):
    """dw slab + slice partials + the token blocks of the two hand-offs + the granule block (t2amd_attn_bwd_ws_floats)."""
    return int(load().t2amd_attn_bwd_ws_floats(int(B), int(Ti)))


def set_attn_bwd_granules(on):
    """First hand-off of the one-launch attention backward: 1 granules, 0 drained stores + token, -1 library default."""
    _check(load().t2amd_set_attn_bwd_granules(int(on)), "t2amd_set_attn_bwd_granules")


def attn_handoff_timeouts(reset=True):
    """Abandoned in-launch hand-offs of the one-launch attention forms since the last reset (synchronises)."""
    n = load().t2amd_attn_handoff_timeouts(1 if reset else 0)
    if n < 0:
        raise NativeError("t2amd_attn_handoff_timeouts failed")
    return n


def set_attn_bwd_fused(on):
    """1: the attention backward of a step as one launch (default), 0: K_b1 / K_b2 as separate launches, -1: default."""
    _check(load().t2amd_set_attn_bwd_fused(int(on)), "t2amd_set_attn_bwd_fused")
    _attn_fused_sel["bwd"] = int(on)


def attention_step_fwd(h, Wq, U, v, pm, memory, lens, w_prev, cum, cum_save, w_out, ctx_out, q_out, ws, active=None,
                       bf16=False, memory16=None, Wq16=None, ctx_x3_out=None):
    """``ctx_x3_out``: a [B][2 E] bfloat16 tensor that receives the split-bf16 image of the context ('bf16x3' mode)."""
    lib = load()
    a = AttnFwd()
    B, Ti, E = memory.shape
    a.B, a.Ti, a.E, a.Hq = B, Ti, E, h.shape[1]
    a.h, a.ld_h = _mat(h)[:2]
    a.Wq, a.U, a.v, a.pm, a.memory = ptr(_fullc(Wq)), ptr(U), ptr(v), ptr(_fullc(pm)), ptr(_fullc(memory))
    a.lens = ptr(lens, torch.int32)
    if w_prev is not None:
        a.w_prev, a.ld_wprev = _mat(w_prev)[:2]
    a.cum = ptr(_fullc(cum))
    a.cum_save = ptr(cum_save)
    a.w_out, a.ld_wout = _mat(w_out)[:2]
    a.ctx_out, a.ld_ctx = _mat(ctx_out)[:2]
    if q_out is not None:
        a.q_out, a.ld_q = _mat(q_out)[:2]
    a.active = ptr(active, torch.uint8)
    if ws.numel() < attn_fwd_ws_floats(B, Ti):
        raise NativeError("attention_step_fwd: workspace too small")
    a.ws = ptr(_fullc(ws))
    a.ws_floats = ws.numel()
    a.loc_split_bf16 = 1 if bf16 else 0
    if memory16 is not None:
        a.memory16 = ptr(_fullc(memory16), torch.bfloat16)
    if Wq16 is not None:
        a.Wq16 = ptr(_fullc(Wq16), torch.bfloat16)
    if ctx_x3_out is not None:
        if tuple(ctx_x3_out.shape) != (B, 2 * E) or E % 16:
            raise NativeError("attention_step_fwd: ctx_x3_out must be [B][2 E] bfloat16, E %% 16 == 0")
        a.ctx16_out, a.ld_ctx16, a.ctx16_x3 = ptr(_fullc(ctx_x3_out), torch.bfloat16), E, 1
    _check(lib.t2amd_attention_step_fwd_f32(C.byref(a), _stream()), "t2amd_attention_step_fwd_f32")


def attention_step_bwd(dctx_list, dctx_total, d_w_extra, q, Wq, U, v, pm, memory, lens, w, w_prev, cum_before,
                       dwin_part, dcum_acc, d_pm, dU_acc, dv_acc, dq_out, dh_parts, ws, bf16=False, memory16=None,
                       cell_q=None, cell_x=None, Wq16=None):
    """dwin_part: (ATT_SLICES, B, 2, Ti) in/out; dcum_acc: (B, Ti) in/out; dh_parts: (ATT_SLICES, B, Hq) out.
    cell_q / cell_x: descriptors of lstm_bwd_desc() to run inside this launch (t2amd_attn_bwd.cell_q / cell_x)."""
    lib = load()
    a = AttnBwd()
    B, Ti, E = memory.shape
    a.B, a.Ti, a.E, a.Hq = B, Ti, E, Wq.shape[1]
    for i in range(3):
        a.dctx[i] = _addend(dctx_list[i] if i < len(dctx_list) else None)
    a.dctx_total, a.ld_dctx_total = _mat(dctx_total)[:2]
    if d_w_extra is not None:
        a.d_w_extra, a.ld_dwextra = _mat(d_w_extra)[:2]
    a.q, a.ld_q = _mat(q)[:2]
    a.Wq, a.U, a.v, a.pm, a.memory = ptr(_fullc(Wq)), ptr(U), ptr(v), ptr(_fullc(pm)), ptr(_fullc(memory))
    a.lens = ptr(lens, torch.int32)
    a.w, a.ld_w = _mat(w)[:2]
    if w_prev is not None:
        a.w_prev, a.ld_wprev = _mat(w_prev)[:2]
    a.cum_before = ptr(_fullc(cum_before))
    if tuple(dwin_part.shape) != (ATT_SLICES, B, 2, Ti) or tuple(dh_parts.shape) != (ATT_SLICES, B, Wq.shape[1]):
        raise NativeError("attention_step_bwd: dwin_part / dh_parts have the wrong shape")
    a.dwin_part, a.dcum_acc = ptr(_fullc(dwin_part)), ptr(_fullc(dcum_acc))
    a.d_pm, a.dU_acc, a.dv_acc = ptr(_fullc(d_pm)), ptr(_fullc(dU_acc)), ptr(_fullc(dv_acc))
    a.dq_out, a.ld_dq = _mat(dq_out)[:2]
    a.dh_out, a.ld_dh, a.dh_split_stride = ptr(_fullc(dh_parts)), Wq.shape[1], B * Wq.shape[1]
    if ws.numel() < attn_bwd_ws_floats(B, Ti):
        raise NativeError("attention_step_bwd: workspace too small")
    a.ws = ptr(_fullc(ws))
    a.ws_floats = ws.numel()
    a.bf16 = 1 if bf16 else 0
    if memory16 is not None:
        a.memory16 = ptr(_fullc(memory16), torch.bfloat16)
    if cell_q is not None:
        a.cell_q = C.pointer(cell_q)
    if cell_x is not None:
        a.cell_x = C.pointer(cell_x)
    if Wq16 is not None:
        a.Wq16 = ptr(_fullc(Wq16), torch.bfloat16)
    _check(lib.t2amd_attention_step_bwd_f32(C.byref(a), _stream()), "t2amd_attention_step_bwd_f32")


# ----------------------------------------------------------------------------
# loops
# ----------------------------------------------------------------------------
# The loop-level entry points are also registered with the PyTorch dispatcher (csrc/torch_ops.cpp, TORCH_LIBRARY over
# the same C ABI: torch.ops.tacotron2_amd.*).  When that library is present the engine's loops go through it -- the
# descriptor travels as a CPU uint8 tensor, the tensors it points into as the op's `reads` / `writes` lists -- otherwise
# (and for the instrumented T2AMD_LIB builds, the validate-only CPU runs, and T2AMD_TORCH_OPS=0) through ctypes.
_torch_ops = None


def torch_ops():
    """torch.ops.tacotron2_amd, or None when the registration library is absent / disabled."""
    global _torch_ops
    if _torch_ops is None:
        ok = (os.environ.get("T2AMD_TORCH_OPS", "1") != "0" and "T2AMD_LIB" not in os.environ
              and os.path.exists(TORCH_OPS_PATH))
        if ok:
            load()                                    # the C ABI library first: the ops library resolves against it
            torch.ops.load_library(TORCH_OPS_PATH)
            _torch_ops = torch.ops.tacotron2_amd
        else:
            _torch_ops = False
    return _torch_ops or None


def _desc_tensor(desc):
    return torch.frombuffer(desc, dtype=torch.uint8)          # zero-copy view of the ctypes struct


def _dev_tensors(ts):
    return [t for t in ts if t is not None and torch.is_tensor(t) and t.is_cuda]


def _via_ops(name, descs, reads, writes):
    """Run loop `name` through the dispatcher when possible; False -> the caller takes the ctypes route."""
    ops = None if _validate_only else torch_ops()
    if ops is None or reads is None or writes is None:
        return False
    w = _dev_tensors(writes)
    if not w:
        return False
    getattr(ops, name)(*[_desc_tensor(d) for d in descs], _dev_tensors(reads), w)
    return True


last_loop_route = None          # 'torch.ops' / 'ctypes': which way the most recent loop-level call went (tests)


def _loop(name, cname, descs, reads, writes):
    global last_loop_route
    if _via_ops(name, descs, reads, writes):
        last_loop_route = 'torch.ops'
        return
    last_loop_route = 'ctypes'
    _check(getattr(load(), cname)(*[C.byref(d) for d in descs], _stream()), cname)


def decoder_train_fwd_loop(desc, reads=None, writes=None):
    _loop("decoder_train_fwd", "t2amd_decoder_train_fwd_loop_f32", [desc], reads, writes)


def decoder_train_bwd_loop(desc, reads=None, writes=None):
    _loop("decoder_train_bwd", "t2amd_decoder_train_bwd_loop_f32", [desc], reads, writes)


def lstm_seq_fwd(desc):
    lib = load()
    _check(lib.t2amd_lstm_seq_fwd_f32(C.byref(desc), _stream()), "t2amd_lstm_seq_fwd_f32")


def lstm_seq_fwd2(d0, d1, reads=None, writes=None):
    _loop("encoder_lstm_fwd", "t2amd_lstm_seq_fwd2_f32", [d0, d1], reads, writes)


def lstm_seq_persistent_supported(desc):
    """None when the encoder bi-LSTM of this geometry can run as one persistent launch, else the reason."""
    lib = load()
    if lib.t2amd_lstm_seq_persistent_supported(C.byref(desc)) == 0:
        return None
    msg = lib.t2amd_last_error()
    return msg.decode() if msg else "unsupported"


def lstm_seq_fwd2_persistent(d0, d1, mailbox, status):
    """Both directions of a single-utterance encoder bi-LSTM as one persistent launch (csrc/decode_persist.hip)."""
    need = load().t2amd_lstm_seq_persistent_mailbox_bytes(d0.H, 2)
    if mailbox.numel() * mailbox.element_size() < need:
        raise NativeError("lstm_seq_fwd2_persistent: mailbox of %d bytes, %d needed" % (mailbox.numel() * mailbox.element_size(), need))
    _check(load().t2amd_lstm_seq_fwd2_persistent_f32(C.byref(d0), C.byref(d1), ptr(mailbox, torch.int64), ptr(status, torch.int32),
                                                     _stream()), "t2amd_lstm_seq_fwd2_persistent_f32")


def decoder_train_fwd_persistent_supported(desc, cus):
    """None when the teacher-forced decoder loop can run as ONE persistent launch on a device of `cus` CUs, else the reason."""
    lib = load()
    if lib.t2amd_decoder_train_fwd_persistent_supported(C.byref(desc), int(cus)) == 0:
        return None
    msg = lib.t2amd_last_error()
    return msg.decode() if msg else "unsupported"


def decoder_train_fwd_persistent_flag_words(B, Ha):
    return int(load().t2amd_decoder_train_fwd_persistent_flag_bytes(int(B), int(Ha))) // 4


def decoder_train_fwd_persistent(desc, flags, status, poison=None):
    """reference model.py:405-411 (the teacher-forced loop) as one persistent launch (csrc/attention.hip,
    dec_train_fwd_persistent_kernel): bit-identical to decoder_train_fwd_loop.  ``poison``: an f32 tensor whose first element
    becomes NaN if a workgroup gave up (for callers that do not read ``status`` back)."""
    lib = load()
    need = lib.t2amd_decoder_train_fwd_persistent_flag_bytes(desc.B, desc.Ha)
    if flags.dtype != torch.int32 or flags.numel() * 4 < need:
        raise NativeError("decoder_train_fwd_persistent: int32 flags of %d bytes needed" % need)
    _check(lib.t2amd_decoder_train_fwd_persistent_f32(C.byref(desc), C.c_void_p(flags.data_ptr()), ptr(status, torch.int32),
                                                      ptr(poison) if poison is not None else None, _stream()),
           "t2amd_decoder_train_fwd_persistent_f32")


def lstm_seq_batch_persistent_supported(desc, ndir, cus):
    """None when the encoder bi-LSTM of this batch can run as one persistent launch on a device of `cus` CUs, else the reason."""
    lib = load()
    if lib.t2amd_lstm_seq_batch_persistent_supported(C.byref(desc), int(ndir), int(cus)) == 0:
        return None
    msg = lib.t2amd_last_error()
    return msg.decode() if msg else "unsupported"


def lstm_seq_batch_persistent_flag_words(B, H, ndir=2):
    return int(load().t2amd_lstm_seq_batch_persistent_flag_bytes(int(B), int(H), int(ndir))) // 4


def lstm_seq_fwd2_batch_persistent(d0, d1, flags, status, poison=None):
    """Both directions of the encoder bi-LSTM of a BATCH as one persistent launch (csrc/decode_persist.hip).  ``poison``: an
    f32 tensor whose first element becomes NaN if a workgroup gave up (for callers that do not read ``status`` back)."""
    lib = load()
    need = lib.t2amd_lstm_seq_batch_persistent_flag_bytes(d0.B, d0.H, 2)
    if flags.numel() * flags.element_size() < need:
        raise NativeError("lstm_seq_fwd2_batch_persistent: flags of %d bytes, %d needed" % (flags.numel() * flags.element_size(), need))
    _check(lib.t2amd_lstm_seq_fwd2_batch_persistent_f32(C.byref(d0), C.byref(d1), C.c_void_p(flags.data_ptr()), ptr(status, torch.int32),
                                                        ptr(poison) if poison is not None else None, _stream()),
           "t2amd_lstm_seq_fwd2_batch_persistent_f32")


def lstm_seq_bwd2_batch_persistent_supported(desc, ndir, cus):
    """None when the encoder bi-LSTM's BPTT of this batch can run as one persistent launch on a device of `cus` CUs, else the reason."""
    lib = load()
    if lib.t2amd_lstm_seq_bwd2_batch_persistent_supported(C.byref(desc), int(ndir), int(cus)) == 0:
        return None
    msg = lib.t2amd_last_error()
    return msg.decode() if msg else "unsupported"


def lstm_seq_bwd2_batch_persistent(d0, d1, flags, status, poison=None):
    """BPTT of both directions of the encoder bi-LSTM of a BATCH as one persistent launch (csrc/decode_persist.hip,
    encoder_bilstm_batch_persistent_bwd_kernel) instead of 2 T dependent launches (lstm_seq_bwd2)."""
    lib = load()
    need = lib.t2amd_lstm_seq_batch_persistent_flag_bytes(d0.B, d0.H, 2)
    if flags.numel() * flags.element_size() < need:
        raise NativeError("lstm_seq_bwd2_batch_persistent: flags of %d bytes, %d needed" % (flags.numel() * flags.element_size(), need))
    _check(lib.t2amd_lstm_seq_bwd2_batch_persistent_f32(C.byref(d0), C.byref(d1), C.c_void_p(flags.data_ptr()), ptr(status, torch.int32),
                                                        ptr(poison) if poison is not None else None, _stream()),
           "t2amd_lstm_seq_bwd2_batch_persistent_f32")


def encoder_handoff_timeouts(reset=True):
    """Give-ups of the batched persistent encoder launch since the last reset (synchronises)."""
    n = load().t2amd_encoder_handoff_timeouts(1 if reset else 0)
    if n < 0:
        raise NativeError("t2amd_encoder_handoff_timeouts failed")
    return n


def lstm_seq_bwd2(d0, d1, reads=None, writes=None):
    _loop("encoder_lstm_bwd", "t2amd_lstm_seq_bwd2_f32", [d0, d1], reads, writes)


def lstm_seq_bwd(desc):
    lib = load()
    _check(lib.t2amd_lstm_seq_bwd_f32(C.byref(desc), _stream()), "t2amd_lstm_seq_bwd_f32")


def decoder_infer_steps(desc, reads=None, writes=None):
    _loop("decoder_infer_steps", "t2amd_decoder_infer_steps_f32", [desc], reads, writes)


# ----------------------------------------------------------------------------
# mel front end (csrc/audio.hip)
# ----------------------------------------------------------------------------
def reflect_index(i, T):
    """Host copy of the kernel's reflect rule (no GPU needed)."""
    return int(load().t2amd_reflect_index(int(i), int(T)))


def reflect_pad(y, out, pad):
    """out[b][:T+2*pad] = reflect-padded y[b]; the rest of each out row is zeroed.  y (B,T), out (B,Tout)."""
    py, ldy, B, T = _mat(y)
    po, ldo, B1, Tout = _mat(out)
    if B1 != B:
        raise NativeError("reflect_pad: batch mismatch %s vs %s" % (tuple(y.shape), tuple(out.shape)))
    _check(load().t2amd_reflect_pad_f32(py, _i64(ldy), po, _i64(ldo), B, T, int(pad), Tout, _stream()),
           "t2amd_reflect_pad_f32")


def stft_magnitude(spec, mag, F):
    """mag[r][:F] = |spec[r][:F] + i spec[r][F:2F]|, mag[r][F:] = 0.  Chunked to the grid limit."""
    ps, lds, R, C2 = _mat(spec)
    pm, ldm, R1, Fpad = _mat(mag)
    if R1 != R or C2 < 2 * F or Fpad < F:
        raise NativeError("stft_magnitude: shape mismatch spec=%s mag=%s F=%d" % (tuple(spec.shape), tuple(mag.shape), F))
    lib = load()
    for r0 in range(0, R, 65535):
        rows = min(65535, R - r0)
        _check(lib.t2amd_stft_magnitude_f32(ptr(spec[r0:]), _i64(lds), ptr(mag[r0:]), _i64(ldm), _i64(rows), int(F),
                                            Fpad, _stream()), "t2amd_stft_magnitude_f32")


def mel_log_compress(mel, out, clip):
    """out (B, n_mel, n) = log(max(mel (B*n, n_mel), clip)) transposed per utterance."""
    pm, ld, R, n_mel = _mat(mel)
    B, n_mel1, n = out.shape
    if n_mel1 != n_mel or B * n != R:
        raise NativeError("mel_log_compress: shape mismatch mel=%s out=%s" % (tuple(mel.shape), tuple(out.shape)))
    _check(load().t2amd_mel_log_compress_f32(pm, _i64(ld), ptr(_fullc(out)), B, n, n_mel, C.c_float(clip), _stream()),
           "t2amd_mel_log_compress_f32")


# ---- the way back and the mel L1 loss (csrc/audio_bwd.hip) ---------------------------------------------------------------
def mel_log_bwd(d_out, mel, d_mel, clip):
    """d_mel (B*n, n_mel) = d_out (B, n_mel, n) transposed per utterance / mel where mel >= clip, 0 elsewhere."""
    pm, ld, R, n_mel = _mat(mel)
    pd, ldd, Rd, n_mel_d = _mat(d_mel)
    if d_out.dim() != 3 or (Rd, n_mel_d) != (R, n_mel) or d_out.shape[1] != n_mel or d_out.shape[0] * d_out.shape[2] != R:
        raise NativeError("mel_log_bwd: shape mismatch d_out=%s mel=%s d_mel=%s" % (tuple(d_out.shape), tuple(mel.shape),
                                                                                  tuple(d_mel.shape)))
    B, _, n = d_out.shape
    _check(load().t2amd_mel_log_bwd_f32(ptr(_fullc(d_out)), pm, _i64(ld), pd, _i64(ldd), B, n, n_mel, C.c_float(clip), _stream()),
           "t2amd_mel_log_bwd_f32")


def stft_magnitude_bwd(d_mag, spec, d_spec, F):
    """d_spec[r] = [d_mag re / mag | d_mag im / mag | 0] from spec[r] = [re (F) | im (F)]; 0 where mag == 0."""
    pg, ldm, R, Fm = _mat(d_mag)
    ps, lds, Rs, C2 = _mat(spec)
    pd, ldd, Rd, Kp = _mat(d_spec)
    if (Rs, Rd) != (R, R) or C2 < 2 * F or Fm < F or Kp < 2 * F:
        raise NativeError("stft_magnitude_bwd: shape mismatch d_mag=%s spec=%s d_spec=%s F=%d"
                          % (tuple(d_mag.shape), tuple(spec.shape), tuple(d_spec.shape), F))
    _check(load().t2amd_stft_magnitude_bwd_f32(pg, _i64(ldm), ps, _i64(lds), pd, _i64(ldd), _i64(R), int(F), int(Kp), _stream()),
           "t2amd_stft_magnitude_bwd_f32")


def stft_frames_fold(d_frames, d_y, hop, pad):
    """d_y (B, T) = the overlap-add of the frame gradients d_frames (B*n, L), n = T // hop + 1, folded back through the reflect
    padding of `pad` samples."""
    pf, ldf, R, L = _mat(d_frames)
    py, ldy, B, T = _mat(d_y)
    n = T // int(hop) + 1
    if R != B * n:
        raise NativeError("stft_frames_fold: %d frame rows for (B, T) = %s at hop %d (%d frames each)" % (R, tuple(d_y.shape), hop, n))
    _check(load().t2amd_stft_frames_fold_f32(pf, _i64(ldf), _i64(_floats(d_frames)), py, _i64(ldy), _i64(_floats(d_y)), B, T, n, L,
                                             int(hop), int(pad), _stream()), "t2amd_stft_frames_fold_f32")


def mel_l1_slots(B, n_mel, n):
    """Partial slots of ``mel_l1_fwd`` for (B, n_mel, n) log-mels."""
    return -(-int(B) * int(n_mel) // int(load().t2amd_mel_l1_rows_per_slot(int(n))))


def _l1_args(who, out, target, lens):
    if out.dim() != 3 or target.dim() != 3 or tuple(target.shape[:2]) != tuple(out.shape[:2]):
        raise NativeError("%s: shape mismatch out=%s target=%s" % (who, tuple(out.shape), tuple(target.shape)))
    B, n_mel, n = out.shape
    if lens is not None and (lens.dtype != torch.int32 or lens.dim() != 1 or lens.numel() != B or not lens.is_contiguous()):
        raise NativeError("%s: lens must be a contiguous int32 vector of %d frame counts" % (who, B))
    return B, n_mel, n, target.shape[2]


def mel_l1_fwd(out, target, lens, count, partial):
    """partial[s] = slot s's share of sum |out - target| / count over the frames i < lens[b] (lens None: all N); out
    (B, n_mel, n), target (B, n_mel, N).  ``wg_partial_sum`` over ``mel_l1_slots`` slots gives the loss."""
    B, n_mel, n, N = _l1_args("mel_l1_fwd", out, target, lens)
    _check(load().t2amd_mel_l1_fwd_f32(ptr(_fullc(out)), ptr(_fullc(target)), None if lens is None else ptr(lens, torch.int32), B,
                                       n_mel, n, N, _i64(int(count)), ptr(_fullc(partial)), _i64(partial.numel()), _stream()),
           "t2amd_mel_l1_fwd_f32")


def mel_l1_bwd(out, target, lens, g, count, d_out):
    """d_out (B, n_mel, n) = sign(out - target) g / count inside the mask, 0 outside; g: a one-element device tensor."""
    B, n_mel, n, N = _l1_args("mel_l1_bwd", out, target, lens)
    if tuple(d_out.shape) != tuple(out.shape) or g.numel() != 1:
        raise NativeError("mel_l1_bwd: d_out %s beside out %s, g of %d elements" % (tuple(d_out.shape), tuple(out.shape), g.numel()))
    _check(load().t2amd_mel_l1_bwd_f32(ptr(_fullc(out)), ptr(_fullc(target)), None if lens is None else ptr(lens, torch.int32),
                                       ptr(_fullc(g)), B, n_mel, n, N, _i64(int(count)), ptr(_fullc(d_out)), _stream()),
           "t2amd_mel_l1_bwd_f32")


# ---- multi-resolution STFT loss (csrc/stft_loss.hip) -----------------------------------------------------------------------
def stft_loss_slots(rows, F):
    """Partial slots (three float64 sums each) of ``stft_loss_fwd`` for `rows` frame rows of F bins."""
    return -(-int(rows) // int(load().t2amd_stft_loss_rows_per_slot(int(F))))


def _stft_loss_args(who, spec_x, spec_y, cnt, n, F):
    px, ldx, R, Cx = _mat(spec_x)
    py, ldy, Ry, Cy = _mat(spec_y)
    n, F = int(n), int(F)
    if Ry != R or Cx < 2 * F or Cy < 2 * F or n < 1 or R % n:
        raise NativeError("%s: shape mismatch spec_x=%s spec_y=%s n=%d F=%d" % (who, tuple(spec_x.shape), tuple(spec_y.shape), n, F))
    B = R // n
    if cnt is None or cnt.dtype != torch.int32 or cnt.dim() != 1 or cnt.numel() != B or not cnt.is_contiguous():
        raise NativeError("%s: cnt must be a contiguous int32 vector of %d frame counts" % (who, B))
    return px, ldx, py, ldy, B


def stft_loss_fwd(spec_x, spec_y, cnt, n, F, eps, slots):
    """slots (float64, 3 per slot) = the partial sums of (m_y - m_x)^2, m_y^2 and |ln m_x - ln m_y| over the frames j < cnt[b];
    spec_x, spec_y (B n, 2F) rows [re | im].  ``stft_loss_finish`` combines them."""
    px, ldx, py, ldy, B = _stft_loss_args("stft_loss_fwd", spec_x, spec_y, cnt, n, F)
    _check(load().t2amd_stft_loss_fwd_f32(px, _i64(ldx), py, _i64(ldy), ptr(cnt, torch.int32), B, int(n), int(F), C.c_float(eps),
                                          ptr(_fullc(slots), torch.float64), _i64(slots.numel()), _stream()),
           "t2amd_stft_loss_fwd_f32")


def stft_loss_finish(slots, offsets, counts, sc_weight, mag_weight, loss, terms, coef):
    """loss (1,), terms (R, 2) = (sc_r, lm_r) and coef (R, 2) from every resolution's slots; ``offsets`` (R + 1 slot indices)
    and ``counts`` (R values C_r) are host lists."""
    R = len(counts)
    if len(offsets) != R + 1 or loss.numel() != 1 or terms.numel() != 2 * R or coef.numel() != 2 * R:
        raise NativeError("stft_loss_finish: %d offsets, %d counts, loss of %d, terms of %d, coef of %d elements"
                          % (len(offsets), R, loss.numel(), terms.numel(), coef.numel()))
    off = (C.c_longlong * (R + 1))(*[int(v) for v in offsets])
    cnt = (C.c_double * max(R, 1))(*[float(v) for v in counts])
    _check(load().t2amd_stft_loss_finish_f64(ptr(_fullc(slots), torch.float64), _i64(slots.numel()), off, cnt, R,
                                             C.c_float(sc_weight), C.c_float(mag_weight), ptr(_fullc(loss)), ptr(_fullc(terms)),
                                             ptr(_fullc(coef)), _stream()), "t2amd_stft_loss_finish_f64")


def stft_loss_bwd(spec_x, spec_y, cnt, coef, g, n, F, eps, d_spec):
    """d_spec (B n, Kp) = [d_re | d_im | 0] of one resolution from its spectra, its two coefficients ``coef`` (2,) and the upstream
    scalar ``g`` (one-element device tensor); 0 below eps and outside the mask."""
    px, ldx, py, ldy, B = _stft_loss_args("stft_loss_bwd", spec_x, spec_y, cnt, n, F)
    pd, ldd, Rd, Kp = _mat(d_spec)
    if Rd != B * int(n) or Kp < 2 * int(F) or coef.numel() != 2 or g.numel() != 1:
        raise NativeError("stft_loss_bwd: shape mismatch d_spec=%s for %d rows of F=%d, coef of %d, g of %d elements"
                          % (tuple(d_spec.shape), B * int(n), F, coef.numel(), g.numel()))
    _check(load().t2amd_stft_loss_bwd_f32(px, _i64(ldx), py, _i64(ldy), ptr(cnt, torch.int32), ptr(_fullc(coef)), ptr(_fullc(g)), B,
                                          int(n), int(F), int(Kp), C.c_float(eps), pd, _i64(ldd), _i64(_floats(d_spec)), _stream()),
           "t2amd_stft_loss_bwd_f32")


def stft_loss_sum(parts, out):
    """out = ((parts[0] + parts[1]) + ...) + parts[R - 1]; parts (R, ...) contiguous, out of one part's shape."""
    R = parts.shape[0]
    if parts.dim() < 2 or tuple(parts.shape[1:]) != tuple(out.shape):
        raise NativeError("stft_loss_sum: parts %s beside out %s" % (tuple(parts.shape), tuple(out.shape)))
    _check(load().t2amd_stft_loss_sum_f32(ptr(_fullc(parts)), _i64(out.numel()), _i64(parts.numel()), int(R), _i64(out.numel()),
                                          ptr(_fullc(out)), _stream()), "t2amd_stft_loss_sum_f32")


# ---- sample-rate conversion (csrc/resample.hip) -----------------------------------------------------------------------------
def resample_plan(P, I, S, Kd):
    """-> (outputs per workgroup, True when the phase table is staged in LDS) of a resample launch with P phases of S taps, input
    period I and first-tap + S <= Kd; NativeError where the library refuses the geometry."""
    npw, lds = C.c_int(0), C.c_int(0)
    _check(load().t2amd_resample_plan(int(P), int(I), int(S), int(Kd), C.byref(npw), C.byref(lds)), "t2amd_resample_plan")
    return npw.value, bool(lds.value)


def _resample_args(who, x, y, lengths, tab, first, phases):
    px, ldx, B, T = _mat(x)
    py, ldy, By, Tout = _mat(y)
    if By != B or tab.dim() != 2 or tab.shape[0] != phases or first.numel() != phases or first.dtype != torch.int32:
        raise NativeError("%s: shape mismatch x=%s y=%s table=%s first=%s for %d phases"
                          % (who, tuple(x.shape), tuple(y.shape), tuple(tab.shape), tuple(first.shape), phases))
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.dim() != 1 or lengths.numel() != B
                                or not lengths.is_contiguous()):
        raise NativeError("%s: lengths must be a contiguous int32 vector of %d sample counts" % (who, B))
    return px, ldx, py, ldy, B, T, Tout


def resample_fwd(x, lengths, y, tab, first, o, n, width):
    """y (B, ceil(n T / o)) = the polyphase gather of x (B, T) with the compact table ``tab`` (n, S) and first-tap indices
    ``first`` (n, int32); x reads as zero at and beyond ``lengths`` (device int32 or None), y is 0 beyond the new lengths."""
    px, ldx, py, ldy, B, T, Tout = _resample_args("resample_fwd", x, y, lengths, tab, first, int(n))
    _check(load().t2amd_resample_fwd_f32(px, _i64(ldx), None if lengths is None else ptr(lengths, torch.int32), B, _i64(T), py,
                                         _i64(ldy), _i64(Tout), ptr(_fullc(tab)), ptr(_fullc(first), torch.int32), int(o), int(n),
                                         int(tab.shape[1]), int(width), _stream()), "t2amd_resample_fwd_f32")


def resample_bwd(d_y, lengths, d_x, btab, bfirst, o, n, wpad, Kd):
    """d_x (B, T) = the adjoint of ``resample_fwd`` applied to d_y (B, ceil(n T / o)) as a gather with the regrouped table ``btab``
    (o, Sb) and ``bfirst`` (o, int32); d_y is not read beyond the new lengths, d_x is 0 at and beyond ``lengths``."""
    px, ldx, py, ldy, B, T, Tout = _resample_args("resample_bwd", d_x, d_y, lengths, btab, bfirst, int(o))
    _check(load().t2amd_resample_bwd_f32(py, _i64(ldy), None if lengths is None else ptr(lengths, torch.int32), B, _i64(T),
                                         _i64(Tout), px, _i64(ldx), ptr(_fullc(btab)), ptr(_fullc(bfirst), torch.int32), int(o),
                                         int(n), int(btab.shape[1]), int(wpad), int(Kd), _stream()), "t2amd_resample_bwd_f32")


# ---- mel-cepstral distortion under dynamic time warping (csrc/dtw.hip) ------------------------------------------------------------
def dtw_width():
    """Rows of a band of the DTW wavefront (the lanes of its workgroup)."""
    return int(load().t2amd_dtw_width())


def _pair_lengths(who, n, B):
    if n is not None and (n.dtype != torch.int32 or n.dim() != 1 or n.numel() != B or not n.is_contiguous()):
        raise NativeError("%s: lengths must be a contiguous int32 vector of %d frame counts" % (who, B))
    return None if n is None else ptr(n, torch.int32)


# ---- argument helpers of the ragged ops: a padded batch, per-utterance lengths, strided float32 operands, a uint8 workspace ----------
# Two stride conventions, because the C entries check two things.  The path, aligner and regulator entries ask for strides that
# cover the matrix (``_cover_strides``); the matrix-pipe entries of self-attention and the FFT block ask for 16-byte bases and
# strides in multiples of 4 floats, and take 0 for an axis of one element (``_operand``).
def _cover(x):
    """(batch stride, row stride) of a rank-3 tensor; an axis of one element gets a stride that covers what it holds."""
    B, R, cols = x.shape
    sr = x.stride(1) if R > 1 else max(x.stride(1), cols)
    sb = x.stride(0) if B > 1 else max(x.stride(0), (R - 1) * sr + cols)
    return sb, sr


def _cover_strides(who, x, what, along):
    """``_cover`` of a rank-3 tensor without an empty axis and with unit stride on its last one; ``what`` names it in the refusal,
    as in "(B, T, N) scores", and ``along`` is the last axis' letter."""
    if x.dim() != 3 or min(x.shape) < 1 or (x.shape[2] > 1 and x.stride(2) != 1):
        raise NativeError("%s: expected %s with unit stride along %s, got shape %s stride %s" % (who, what, along, tuple(x.shape), x.stride()))
    return _cover(x)


def _operand(who, x, name, axes, shape=None):
    """[pointer, stride of every axis but the last] of a float32 tensor of the rank ``axes`` spells out, "(B, T, H, D)" or
    "(B, T, C)", with unit stride along the last axis; an axis of one element has no stride."""
    n = axes.count(",")
    if x.dim() != n + 1 or min(x.shape) < 1 or x.stride(n) != 1 or (shape is not None and tuple(x.shape) != tuple(shape)):
        raise NativeError("%s: expected %s %s%s with unit stride along %s, got shape %s stride %s"
                          % (who, name, axes, "" if shape is None else " = %s" % (tuple(shape),), axes[-2], tuple(x.shape), x.stride()))
    return [ptr(x)] + [_i64(x.stride(i) if x.shape[i] > 1 else 0) for i in range(n)]


def _exact(who, t, name, shape, dtype=None):
    """Pointer of ``t``: None, or a contiguous tensor of exactly ``shape``.  The integer operands name their ``dtype`` and the
    refusal says which came instead; without one ``t`` is float32, and a wrong dtype is ``ptr``'s to refuse."""
    if t is None:
        return None
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or (dtype is not None and t.dtype != dtype):
        if dtype is None:
            raise NativeError("%s: expected contiguous %s %s, got shape %s stride %s" % (who, name, tuple(shape), tuple(t.shape), t.stride()))
        raise NativeError("%s: expected contiguous %s %s of shape %s, got %s %s"
                          % (who, str(dtype).replace("torch.", ""), name, tuple(shape), t.dtype, tuple(t.shape)))
    return ptr(t, dtype or torch.float32)


def _workspace(who, ws):
    """(pointer, bytes) of a workspace: a contiguous uint8 tensor."""
    if ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise NativeError("%s: the workspace must be a contiguous uint8 tensor, got %s" % (who, ws.dtype))
    return ptr(ws, torch.uint8), _i64(ws.numel())


def _query_ints(entry, n, *args):
    """The n ints the C query ``entry`` writes behind its arguments."""
    v = [C.c_int(0) for _ in range(n)]
    _check(getattr(load(), entry)(*args, *[C.byref(x) for x in v]), entry)
    return tuple(x.value for x in v)


def _query_bytes(entry, *args):
    """The one long long (a workspace's bytes) the C query ``entry`` writes behind its arguments."""
    n = C.c_longlong(0)
    _check(getattr(load(), entry)(*args, C.byref(n)), entry)
    return n.value


def mel_cepstrum(mel, lengths, basis, out):
    """out (B, T, K) = the cepstra of the log-mel ``mel`` (B, n_mel, T) (unit stride along T) under ``basis`` (K, n_mel); rows at
    and beyond ``lengths`` (device int32 or None) are zeros."""
    if mel.dim() != 3 or basis.dim() != 2 or out.dim() != 3 or (mel.shape[2] > 1 and mel.stride(2) != 1) \
            or basis.shape[1] != mel.shape[1] or tuple(out.shape) != (mel.shape[0], mel.shape[2], basis.shape[0]):
        raise NativeError("mel_cepstrum: shape mismatch mel=%s stride %s basis=%s out=%s"
                          % (tuple(mel.shape), mel.stride(), tuple(basis.shape), tuple(out.shape)))
    B, N, T = mel.shape
    ldb, ldm = _cover(mel)
    _check(load().t2amd_mel_cepstrum_f32(ptr(mel), _i64(ldb), _i64(ldm), _pair_lengths("mel_cepstrum", lengths, B), B, N, T,
                                         ptr(_fullc(basis)), int(basis.shape[0]), ptr(_fullc(out)), _stream()),
           "t2amd_mel_cepstrum_f32")


def _dtw_slab(who, slab, B):
    if slab.dtype != torch.uint8 or slab.dim() != 3 or slab.shape[0] != B or not slab.is_contiguous():
        raise NativeError("%s: the predecessor slab must be a contiguous (B, rows, cols) uint8 tensor, got %s %s"
                          % (who, slab.dtype, tuple(slab.shape)))
    return ptr(slab, torch.uint8), int(slab.shape[1]), int(slab.shape[2])


def dtw(a, b, na, nb, cost, steps, slab=None):
    """cost (B,) float32 and steps (B,) int32 of the DTW of a (B, Ta, K) against b (B, Tb, K) (both contiguous) with ``na``, ``nb``
    frames (device int32 or None); ``slab`` (B, rows, cols) uint8 receives the chosen predecessor of every cell when given."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or cost.numel() != a.shape[0] \
            or steps.numel() != a.shape[0]:
        raise NativeError("dtw: shape mismatch a=%s b=%s cost=%s steps=%s"
                          % (tuple(a.shape), tuple(b.shape), tuple(cost.shape), tuple(steps.shape)))
    B, Ta, K = a.shape
    Tb = b.shape[1]
    ps, rows, cols = (None, 0, 0) if slab is None else _dtw_slab("dtw", slab, B)
    _check(load().t2amd_dtw_f32(ptr(_fullc(a)), _i64(Ta * K), ptr(_fullc(b)), _i64(Tb * K), _pair_lengths("dtw", na, B),
                                _pair_lengths("dtw", nb, B), B, Ta, Tb, K, ptr(_fullc(cost)), ptr(_fullc(steps), torch.int32), ps,
                                rows, cols, _stream()), "t2amd_dtw_f32")


def dtw_backtrack(slab, na, nb, steps, Ta, Tb, out):
    """out (B, L, 2) int32 = the paths the predecessor bytes of ``dtw`` describe, forward, -1 beyond ``steps``."""
    B = steps.numel()
    ps, rows, cols = _dtw_slab("dtw_backtrack", slab, B)
    if out.dim() != 3 or out.shape[0] != B or out.shape[2] != 2:
        raise NativeError("dtw_backtrack: expected a (B, L, 2) path tensor, got %s" % (tuple(out.shape),))
    _check(load().t2amd_dtw_backtrack(ps, rows, cols, _pair_lengths("dtw_backtrack", na, B), _pair_lengths("dtw_backtrack", nb, B),
                                      ptr(_fullc(steps), torch.int32), B, int(Ta), int(Tb), ptr(_fullc(out), torch.int32),
                                      int(out.shape[1]), _stream()), "t2amd_dtw_backtrack")


# ---- F0 extraction by YIN (csrc/yin.hip) -------------------------------------------------------------------------------------------
def yin_plan(sr, frame_length, hop_length, fmin, fmax):
    """-> (tau_min, tau_max) = (floor(sr / fmax), ceil(sr / fmin)) of a YIN geometry; NativeError where the library refuses it."""
    return _query_ints("t2amd_yin_plan", 2, float(sr), int(frame_length), int(hop_length), float(fmin), float(fmax))


def yin(x, lengths, frame_length, hop_length, tau_min, tau_max, sr, threshold, f0, voiced, aperiodicity, dprime=None):
    """f0, aperiodicity (B, frames) float32 and voiced (B, frames) uint8 of the signals x (B, T) (unit stride along T), frames =
    T // hop_length + 1, zeros at and beyond the ``lengths[b] // hop_length + 1`` frames of utterance b (device int32 or None);
    ``dprime`` (B, frames, tau_max + 2) float32 receives d'(0 .. tau_max + 1) when given."""
    px, ldx, B, T = _mat(x)
    frames = T // max(int(hop_length), 1) + 1
    for name, t, dt in (("f0", f0, torch.float32), ("voiced", voiced, torch.uint8), ("aperiodicity", aperiodicity, torch.float32)):
        if tuple(t.shape) != (B, frames) or t.dtype != dt:
            raise NativeError("yin: %s must be a (%d, %d) %s tensor, got %s %s" % (name, B, frames, dt, tuple(t.shape), t.dtype))
    if dprime is not None and tuple(dprime.shape) != (B, frames, int(tau_max) + 2):
        raise NativeError("yin: the d' slab must be (%d, %d, %d), got %s" % (B, frames, int(tau_max) + 2, tuple(dprime.shape)))
    _check(load().t2amd_yin_f32(px, _i64(ldx), _pair_lengths("yin", lengths, B), B, _i64(T), frames, int(frame_length),
                                int(hop_length), int(tau_min), int(tau_max), float(sr), float(threshold), ptr(_fullc(f0)),
                                ptr(_fullc(voiced), torch.uint8), ptr(_fullc(aperiodicity)),
                                None if dprime is None else ptr(_fullc(dprime)), _stream()), "t2amd_yin_f32")


# ---- forced alignment: the best monotonic path (csrc/align.hip) ------------------------------------------------------------------
def align_limits():
    """-> (lanes of the workgroup, frames at most, tokens at most) of ``monotonic_align``."""
    return _query_ints("t2amd_align_limits", 3)


def align_workspace(B, T_max, N_max):
    """Bytes of the workspace ``monotonic_align`` needs for B utterances of at most T_max frames and N_max tokens."""
    return _query_bytes("t2amd_align_workspace", int(B), int(T_max), int(N_max))


def monotonic_align(scores, t_len, n_len, durations, score, path, ws):
    """durations (B, N) int32, score (B,) float32 and, unless None, path (B, T) int32 of the best monotonic path through each
    scores[b, :t_len[b], :n_len[b]] of the (B, T, N) float32 ``scores`` (unit stride along N; device int32 lengths); ``ws`` is a
    uint8 tensor of at least ``align_workspace(B, T, N)`` bytes."""
    who = "monotonic_align"
    sb, st = _cover_strides(who, scores, "(B, T, N) scores", "N")
    B, T, N = scores.shape
    if tuple(durations.shape) != (B, N) or score.numel() != B or (path is not None and tuple(path.shape) != (B, T)):
        raise NativeError("monotonic_align: expected durations (%d, %d), score (%d,) and path (%d, %d), got %s, %s and %s"
                          % (B, N, B, B, T, tuple(durations.shape), tuple(score.shape), None if path is None else tuple(path.shape)))
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_monotonic_align_f32(ptr(scores), _i64(sb), _i64(st), _pair_lengths(who, t_len, B), _pair_lengths(who, n_len, B),
                                            B, T, N, ptr(_fullc(durations), torch.int32), ptr(_fullc(score)),
                                            None if path is None else ptr(_fullc(path), torch.int32), pw, nw, _stream()),
           "t2amd_monotonic_align_f32")


# ---- forward-sum alignment likelihood and its gradient (csrc/forward_sum.hip) ---------------------------------------------------
_BTN = ("a (B, T, N) tensor", "N")                                         # how the forward-sum and aligner refusals name a matrix


def forward_sum_workspace(B, T_max, N_max, keep=True):
    """Bytes of the workspace ``forward_sum`` needs for B utterances of at most T_max frames and N_max tokens; with ``keep`` it
    holds the alpha rows ``forward_sum_backward`` reads."""
    return _query_bytes("t2amd_forward_sum_workspace", int(B), int(T_max), int(N_max), 1 if keep else 0)


def forward_sum(scores, t_len, n_len, log_z, ws, keep=True):
    """log_z (B,) float32 = the log of the summed probability of all monotonic paths through each scores[b, :t_len[b], :n_len[b]]
    of the (B, T, N) float32 ``scores`` (unit stride along N; device int32 lengths); ``ws`` is a uint8 tensor of at least
    ``forward_sum_workspace(B, T, N, keep)`` bytes, and with ``keep`` it leaves holding what ``forward_sum_backward`` reads."""
    sb, st = _cover_strides("forward_sum", scores, *_BTN)
    B, T, N = scores.shape
    if log_z.numel() != B:
        raise NativeError("forward_sum: expected log_z (%d,), got %s" % (B, tuple(log_z.shape)))
    pw, nw = _workspace("forward_sum", ws)
    _check(load().t2amd_forward_sum_f32(ptr(scores), _i64(sb), _i64(st), _pair_lengths("forward_sum", t_len, B),
                                        _pair_lengths("forward_sum", n_len, B), B, T, N, ptr(_fullc(log_z)), 1 if keep else 0,
                                        pw, nw, _stream()), "t2amd_forward_sum_f32")


def forward_sum_backward(scores, t_len, n_len, log_z, scale, grad, soft, ws):
    """grad (B, T, N) float32 (unit stride along N) = scale[b] (None: 1) times the posterior occupancy of every cell, zeros in an
    utterance's padding, and, unless None, soft (B, N) float32 = its column sums; ``scores``, the lengths, ``log_z`` and ``ws``
    are those of a ``forward_sum(..., keep=True)`` call."""
    sb, st = _cover_strides("forward_sum_backward", scores, *_BTN)
    gb, gt = _cover_strides("forward_sum_backward", grad, *_BTN)
    B, T, N = scores.shape
    if tuple(grad.shape) != (B, T, N) or log_z.numel() != B or (scale is not None and scale.numel() != B) \
            or (soft is not None and tuple(soft.shape) != (B, N)):
        raise NativeError("forward_sum_backward: expected grad (%d, %d, %d), log_z and scale (%d,) and soft (%d, %d), got %s, %s, %s "
                          "and %s" % (B, T, N, B, B, N, tuple(grad.shape), tuple(log_z.shape),
                                      None if scale is None else tuple(scale.shape), None if soft is None else tuple(soft.shape)))
    pw, nw = _workspace("forward_sum_backward", ws)
    _check(load().t2amd_forward_sum_bwd_f32(ptr(scores), _i64(sb), _i64(st), _pair_lengths("forward_sum_backward", t_len, B),
                                            _pair_lengths("forward_sum_backward", n_len, B), B, T, N, ptr(_fullc(log_z)),
                                            None if scale is None else ptr(_fullc(scale)), ptr(grad), _i64(gb), _i64(gt),
                                            None if soft is None else ptr(_fullc(soft)), pw, nw, _stream()),
           "t2amd_forward_sum_bwd_f32")


# ---- learned-aligner scores and their gradient (csrc/aligner.hip, csrc/aligner_rows.hip) ------------------------------------------
def aligner_workspace(B, T_max, N_max, C_, which=0):
    """Bytes of a workspace of the aligner scores for B utterances of at most T_max frames and N_max tokens of C_ channels:
    ``which`` 0 the forward's, 1 the forward's with what the backward reads kept, 2 the backward's own."""
    return _query_bytes("t2amd_aligner_workspace", int(B), int(T_max), int(N_max), int(C_), int(which))


def _aligner_operands(who, q, k):
    if q.dim() != 3 or k.dim() != 3 or min(q.shape) < 1 or min(k.shape) < 1 or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise NativeError("%s: expected queries (B, T, C) and keys (B, N, C), got %s and %s" % (who, tuple(q.shape), tuple(k.shape)))
    return q.shape[0], q.shape[1], k.shape[1], q.shape[2]


def aligner_scores(q, k, t_len, n_len, tau, log_prior, scores, ws, keep=False):
    """scores (B, T, N) float32 (unit stride along N) = log_softmax over the tokens of -tau |q_t - k_n|^2, plus ``log_prior``
    (B, T, N) or None, -inf in every utterance's padding; q (B, T, C) and k (B, N, C) contiguous float32, device int32 lengths;
    ``ws`` is a uint8 tensor of at least ``aligner_workspace(B, T, N, C, keep)`` bytes, and with ``keep`` it leaves holding what
    ``aligner_scores_backward`` reads."""
    who = "aligner_scores"
    B, T, N, C_ = _aligner_operands(who, q, k)
    if tuple(scores.shape) != (B, T, N) or (log_prior is not None and tuple(log_prior.shape) != (B, T, N)):
        raise NativeError("aligner_scores: expected scores and log_prior (%d, %d, %d), got %s and %s"
                          % (B, T, N, tuple(scores.shape), None if log_prior is None else tuple(log_prior.shape)))
    sb, st = _cover_strides(who, scores, *_BTN)
    pb, pt = (0, 0) if log_prior is None else _cover_strides(who, log_prior, *_BTN)
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_aligner_scores_f32(ptr(_fullc(q)), ptr(_fullc(k)), _pair_lengths(who, t_len, B), _pair_lengths(who, n_len, B),
                                           B, T, N, C_, float(tau), ptr(log_prior), _i64(pb), _i64(pt), ptr(scores), _i64(sb), _i64(st),
                                           1 if keep else 0, pw, nw, _stream()), "t2amd_aligner_scores_f32")


def aligner_scores_backward(q, k, t_len, n_len, tau, grad, dq, dk, dlogp, kept, ws):
    """dq (B, T, C), dk (B, N, C) contiguous float32 and, unless None, dlogp (B, T, N) from ``grad`` = dL/dscores (B, T, N) (unit
    stride along N), exact zeros in every utterance's padding; ``kept`` is the workspace of an ``aligner_scores(..., keep=True)``
    call on the same operands, ``ws`` a uint8 tensor of at least ``aligner_workspace(B, T, N, C, 2)`` bytes."""
    who = "aligner_scores_backward"
    B, T, N, C_ = _aligner_operands(who, q, k)
    if tuple(grad.shape) != (B, T, N) or tuple(dq.shape) != (B, T, C_) or tuple(dk.shape) != (B, N, C_) \
            or (dlogp is not None and tuple(dlogp.shape) != (B, T, N)):
        raise NativeError("aligner_scores_backward: expected grad and dlogp (%d, %d, %d), dq (%d, %d, %d) and dk (%d, %d, %d), got "
                          "%s, %s, %s and %s" % (B, T, N, B, T, C_, B, N, C_, tuple(grad.shape),
                                                 None if dlogp is None else tuple(dlogp.shape), tuple(dq.shape), tuple(dk.shape)))
    gb, gt = _cover_strides(who, grad, *_BTN)
    db, dt = (0, 0) if dlogp is None else _cover_strides(who, dlogp, *_BTN)
    pk, nk = _workspace(who, kept)
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_aligner_scores_bwd_f32(ptr(_fullc(q)), ptr(_fullc(k)), _pair_lengths(who, t_len, B), _pair_lengths(who, n_len, B),
                                               B, T, N, C_, float(tau), ptr(grad), _i64(gb), _i64(gt), ptr(_fullc(dq)), ptr(_fullc(dk)),
                                               ptr(dlogp), _i64(db), _i64(dt), pk, nk, pw, nw, _stream()), "t2amd_aligner_scores_bwd_f32")


def beta_binomial_log_prior(t_len, n_len, scaling, out):
    """out (B, T, N) contiguous float32 = the beta-binomial log prior of every frame over the tokens of utterance b (device int32
    lengths), evaluated in float64 and rounded once; -inf in the padding."""
    if out.dim() != 3 or min(out.shape) < 1:
        raise NativeError("beta_binomial_log_prior: expected a (B, T, N) tensor, got %s" % (tuple(out.shape),))
    B, T, N = out.shape
    _check(load().t2amd_beta_binomial_log_prior_f32(_pair_lengths("beta_binomial_log_prior", t_len, B),
                                                    _pair_lengths("beta_binomial_log_prior", n_len, B), B, T, N, float(scaling),
                                                    ptr(_fullc(out)), _stream()), "t2amd_beta_binomial_log_prior_f32")


# ---- the length regulator: durations -> path, expansion, pooling and their gradients (csrc/regulate.hip) --------------------------
def regulate_limits():
    """-> (channels at most, tokens at most, frames at most) of the length regulator."""
    return _query_ints("t2amd_regulate_limits", 3)


def durations_to_path(durations, n_len, T, path, t_lengths, ends=None, totals=None):
    """From the (B, N) int32 or int64 ``durations`` (unit stride along N) and the device int32 token counts ``n_len`` (None: N):
    t_lengths (B,) int32 = min(sum of the durations, T) and, unless None, path (B, T) int32 (the token of every frame, -1 at and
    beyond t_lengths), ends (B, N) int32 (the inclusive prefix sums clamped to T) and totals (B,) int64 (the sums themselves).
    An utterance with a negative duration leaves with t_lengths = totals = -1 and no frames."""
    who = "durations_to_path"
    if durations.dim() != 2 or min(durations.shape) < 1 or (durations.shape[1] > 1 and durations.stride(1) != 1) \
            or durations.dtype not in (torch.int32, torch.int64):
        raise NativeError("%s: expected (B, N) int32 or int64 durations with unit stride along N, got %s shape %s stride %s"
                          % (who, durations.dtype, tuple(durations.shape), durations.stride()))
    B, N = durations.shape
    db = durations.stride(0) if B > 1 else max(durations.stride(0), N)
    if totals is not None and (totals.dtype != torch.int64 or tuple(totals.shape) != (B,) or not totals.is_contiguous()):
        raise NativeError("%s: expected contiguous int64 totals of shape (%d,)" % (who, B))
    _check(load().t2amd_durations_to_path_i32(ptr(durations, None), durations.element_size(), _i64(db), _pair_lengths(who, n_len, B),
                                              B, N, int(T), _exact(who, path, "path", (B, int(T)), torch.int32),
                                              _exact(who, t_lengths, "t_lengths", (B,), torch.int32),
                                              _exact(who, ends, "ends", (B, N), torch.int32),
                                              None if totals is None else ptr(totals, torch.int64), _stream()),
           "t2amd_durations_to_path_i32")


def length_regulate(x, path, y):
    """y (B, T, C) contiguous float32: y[b, t] = x[b, path[b, t]], +0 where path is -1; x (B, N, C), unit stride along C."""
    who = "length_regulate"
    xb, xn = _cover_strides(who, x, "(B, rows, C) tokens", "C")
    B, N, C_ = x.shape
    if y.dim() != 3 or y.shape[0] != B or y.shape[2] != C_ or tuple(path.shape) != tuple(y.shape[:2]):
        raise NativeError("length_regulate: expected y (%d, T, %d) and path (%d, T), got %s and %s"
                          % (B, C_, B, tuple(y.shape), tuple(path.shape)))
    T = y.shape[1]
    _check(load().t2amd_length_regulate_f32(ptr(x), _i64(xb), _i64(xn), _exact(who, path, "path", (B, T), torch.int32), B, N, T, C_,
                                            ptr(_fullc(y)), _stream()), "t2amd_length_regulate_f32")


def length_regulate_backward(dy, ends, dx):
    """dx (B, N, C) contiguous float32: the sum of dy (B, T, C) (unit stride along C) over each token's frames, ascending; ``ends``
    (B, N) int32 as ``durations_to_path`` wrote it."""
    who = "length_regulate_backward"
    gb, gt = _cover_strides(who, dy, "(B, rows, C) gradient", "C")
    B, T, C_ = dy.shape
    if dx.dim() != 3 or dx.shape[0] != B or dx.shape[2] != C_:
        raise NativeError("length_regulate_backward: expected dx (%d, N, %d), got %s" % (B, C_, tuple(dx.shape)))
    N = dx.shape[1]
    _check(load().t2amd_length_regulate_bwd_f32(ptr(dy), _i64(gb), _i64(gt), _exact(who, ends, "ends", (B, N), torch.int32), B, N, T, C_,
                                                ptr(_fullc(dx)), _stream()), "t2amd_length_regulate_bwd_f32")


def _regulate_weights(who, w, B, T):
    if w is None:
        return None, 0
    if w.dim() != 2 or tuple(w.shape) != (B, T) or (T > 1 and w.stride(1) != 1):
        raise NativeError("%s: expected (%d, %d) weights with unit stride along T, got shape %s stride %s"
                          % (who, B, T, tuple(w.shape), w.stride()))
    return ptr(w), (w.stride(0) if B > 1 else max(w.stride(0), T))


def token_average(values, weights, ends, mean, den, num=None):
    """mean (B, N, C) and den (B, N) contiguous float32, and unless None num (B, N, C): the weighted sums of values (B, T, C) (unit
    stride along C) over each token's frames, the sums of the weights (B, T) (None: ones), and their quotient (+0 where den = 0)."""
    who = "token_average"
    vb, vt = _cover_strides(who, values, "(B, rows, C) values", "C")
    B, T, C_ = values.shape
    if mean.dim() != 3 or mean.shape[0] != B or mean.shape[2] != C_ or tuple(den.shape) != tuple(mean.shape[:2]) \
            or (num is not None and tuple(num.shape) != tuple(mean.shape)):
        raise NativeError("%s: expected mean and num (%d, N, %d) and den (%d, N), got %s, %s and %s"
                          % (who, B, C_, B, tuple(mean.shape), None if num is None else tuple(num.shape), tuple(den.shape)))
    N = mean.shape[1]
    pw, wb = _regulate_weights(who, weights, B, T)
    _check(load().t2amd_token_average_f32(ptr(values), _i64(vb), _i64(vt), pw, _i64(wb), _exact(who, ends, "ends", (B, N), torch.int32),
                                          B, N, T, C_, ptr(_fullc(mean)), ptr(_fullc(den)), None if num is None else ptr(_fullc(num)),
                                          _stream()), "t2amd_token_average_f32")


def token_average_backward(grad, den, weights, path, dv):
    """dv (B, T, C) contiguous float32 = weights[b, t] * (grad[b, path[b, t]] / den[b, path[b, t]]), +0 where path is -1 or den is 0;
    grad (B, N, C) and den (B, N) contiguous."""
    who = "token_average_backward"
    if grad.dim() != 3 or dv.dim() != 3 or min(grad.shape) < 1 or min(dv.shape) < 1 or grad.shape[0] != dv.shape[0] \
            or grad.shape[2] != dv.shape[2] or tuple(den.shape) != tuple(grad.shape[:2]):
        raise NativeError("%s: expected grad (B, N, C), den (B, N) and dv (B, T, C), got %s, %s and %s"
                          % (who, tuple(grad.shape), tuple(den.shape), tuple(dv.shape)))
    B, N, C_ = grad.shape
    T = dv.shape[1]
    pw, wb = _regulate_weights(who, weights, B, T)
    _check(load().t2amd_token_average_bwd_f32(ptr(_fullc(grad)), ptr(_fullc(den)), pw, _i64(wb),
                                              _exact(who, path, "path", (B, T), torch.int32), B, N, T, C_, ptr(_fullc(dv)), _stream()),
           "t2amd_token_average_bwd_f32")


# ---- masked multi-head self-attention and its gradient (csrc/self_attn.hip, csrc/self_attn_rows.hip) -----------------------------
_BTHD = "(B, T, H, D)"


def self_attn_limits():
    """-> (frames at most, heads at most, least head width, greatest head width, utterances times heads at most)."""
    return _query_ints("t2amd_self_attn_limits", 5)


def self_attn_workspace(B, T, H, D, which=0):
    """Bytes for B utterances of at most T frames, H heads of width D: ``which`` 0 the forward's workspace (none), 1 the lse the
    forward keeps for a backward, 2 the backward's workspace."""
    return _query_bytes("t2amd_self_attn_workspace", int(B), int(T), int(H), int(D), int(which))


def self_attn(q, k, v, lengths, scale, o, lse=None):
    """o (B, T, H, D) contiguous float32 = softmax(scale q k^T) v per head over each utterance's own ``lengths[b]`` frames (device
    int32, clamped; None: T), +0 at and beyond them; q, k, v (B, T, H, D) float32 with unit stride along D, the other strides
    multiples of 4 floats and 16-byte bases; ``lse`` (B, H, T) or None receives the row logsumexp a backward reads."""
    who = "self_attn"
    aq = _operand(who, q, "q", _BTHD)
    B, T, H, D = q.shape
    ak, av = _operand(who, k, "k", _BTHD, q.shape), _operand(who, v, "v", _BTHD, q.shape)
    _operand(who, o, "o", _BTHD, q.shape)
    _check(load().t2amd_self_attn_f32(*(aq + ak + av + [_pair_lengths(who, lengths, B), B, T, H, D, float(scale), ptr(_fullc(o)),
                                                         _exact(who, lse, "lse", (B, H, T)), _stream()])),
           "t2amd_self_attn_f32")


def self_attn_delta(g, o, lengths, delta):
    """delta (B, H, T) contiguous float32 = sum_d g o per row, +0 at and beyond an utterance's frames: the backward's row pass."""
    who = "self_attn_delta"
    ag = _operand(who, g, "the gradient", _BTHD)
    B, T, H, D = g.shape
    _operand(who, o, "o", _BTHD, g.shape)
    _check(load().t2amd_self_attn_delta_f32(*(ag + [ptr(_fullc(o)), _pair_lengths(who, lengths, B), B, T, H, D,
                                                     _exact(who, delta, "delta", (B, H, T)), _stream()])),
           "t2amd_self_attn_delta_f32")


def self_attn_backward(q, k, v, o, lse, g, lengths, scale, dq, dk, dv, ws):
    """dq, dk, dv (B, T, H, D) contiguous float32 from ``g`` = dL/do (strided as q, k, v may be); ``o`` and ``lse`` are those of a
    ``self_attn`` call on the same operands, ``ws`` a uint8 tensor of at least ``self_attn_workspace(B, T, H, D, 2)`` bytes."""
    who = "self_attn_backward"
    aq = _operand(who, q, "q", _BTHD)
    B, T, H, D = q.shape
    ak, av = _operand(who, k, "k", _BTHD, q.shape), _operand(who, v, "v", _BTHD, q.shape)
    ag = _operand(who, g, "the gradient", _BTHD, q.shape)
    for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        _operand(who, t, name, _BTHD, q.shape)
        _fullc(t)
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_self_attn_bwd_f32(*(aq + ak + av + [ptr(o), _exact(who, lse, "lse", (B, H, T))] + ag
                                            + [_pair_lengths(who, lengths, B), B, T, H, D, float(scale), ptr(dq), ptr(dk), ptr(dv),
                                               pw, nw, _stream()])), "t2amd_self_attn_bwd_f32")


# ---- the feed-forward Transformer block's convolutional feed-forward and add + LayerNorm (csrc/fft_block.hip, fft_block_rows.hip) ----
def fft_block_limits():
    """-> (frames at most, channels at most, kernel width at most, least LayerNorm width, utterances at most)."""
    return _query_ints("t2amd_fft_block_limits", 5)


def fft_block_workspace(B, T, Cin, Cout, k, which):
    """Bytes for B utterances of at most T frames: ``which`` 0 a convolution (none), 1 its weight gradient (the transposed
    gradient slab and the slices' partial sums), 2 the column sums over Cout channels."""
    return _query_bytes("t2amd_fft_block_workspace", int(B), int(T), int(Cin), int(Cout), int(k), int(which))


def ffb_conv(x, image, bias, mask, lengths, k, relu, y):
    """y (B, T, Cout) contiguous = the ragged convolution of x (B, T, Cin) (unit channel stride) under the tap-major weight
    ``image`` (Cout, k Cin), every utterance alone over its own ``lengths[b]`` frames (device int32, clamped; None: T), +0 at and
    beyond them; ``bias`` (Cout) or None, ``relu``, and ``mask`` (B, T, Cout) or None: y is kept only where mask > 0."""
    who = "ffb_conv"
    ax = _operand(who, x, "x", "(B, T, C)")
    B, T, Cin = x.shape
    Cout = y.shape[2] if y.dim() == 3 else -1
    _check(load().t2amd_ffb_conv_f32(*(ax + [_exact(who, image, "the weight image", (Cout, k * Cin)), _exact(who, bias, "bias", (Cout,)),
                                              _exact(who, mask, "mask", (B, T, Cout)), _pair_lengths(who, lengths, B), B, T, Cin, Cout,
                                              int(k), int(bool(relu)), _exact(who, y, "y", (B, T, Cout)), _stream()])),
           "t2amd_ffb_conv_f32")


def ffb_conv_dw(g, x, lengths, k, dw, ws):
    """dw (Cout, Cin, k) contiguous = sum over b then t of g(b, t, o) x(b, t + j - k // 2, i); g (B, T, Cout) contiguous, ``ws`` a
    uint8 tensor of at least ``fft_block_workspace(B, T, Cin, Cout, k, 1)`` bytes."""
    who = "ffb_conv_dw"
    ax = _operand(who, x, "x", "(B, T, C)")
    B, T, Cin = x.shape
    Cout = g.shape[2] if g.dim() == 3 else -1
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_ffb_conv_dw_f32(*([_exact(who, g, "g", (B, T, Cout))] + ax
                                          + [_pair_lengths(who, lengths, B), B, T, Cin, Cout, int(k),
                                             _exact(who, dw, "dw", (Cout, Cin, k)), pw, nw, _stream()])), "t2amd_ffb_conv_dw_f32")


def _ffb_shape(who, x, name):
    if x.dim() != 3:
        raise NativeError("%s: expected %s (B, T, C), got %s" % (who, name, tuple(x.shape)))
    return x.shape


def ffb_add_ln(x, residual, weight, bias, lengths, eps, y, z=None, mean=None, rstd=None):
    """y = LayerNorm(x + residual) weight + bias over the last axis of (B, T, C) on the rows below ``lengths``, +0 beyond;
    ``weight`` None: y = x + residual ("add and mask").  ``z`` (B, T, C), ``mean`` and ``rstd`` (B, T) are kept where given."""
    who = "ffb_add_ln"
    B, T, C_ = _ffb_shape(who, x, "x")
    _check(load().t2amd_ffb_add_ln_f32(_exact(who, x, "x", x.shape), _exact(who, residual, "residual", x.shape),
                                       _exact(who, weight, "weight", (C_,)), _exact(who, bias, "bias", (C_,)),
                                       _pair_lengths(who, lengths, B), B, T, C_, float(eps), _exact(who, y, "y", x.shape),
                                       _exact(who, z, "z", x.shape), _exact(who, mean, "mean", (B, T)),
                                       _exact(who, rstd, "rstd", (B, T)), _stream()), "t2amd_ffb_add_ln_f32")


def ffb_add_ln_backward(g, z, mean, rstd, weight, lengths, dz):
    """dz (B, T, C) = the LayerNorm input gradient of g from the kept z, mean and rstd."""
    who = "ffb_add_ln_backward"
    B, T, C_ = _ffb_shape(who, z, "z")
    _check(load().t2amd_ffb_add_ln_bwd_f32(_exact(who, g, "g", z.shape), _exact(who, z, "z", z.shape),
                                           _exact(who, mean, "mean", (B, T)), _exact(who, rstd, "rstd", (B, T)),
                                           _exact(who, weight, "weight", (C_,)), _pair_lengths(who, lengths, B), B, T, C_,
                                           _exact(who, dz, "dz", z.shape), _stream()), "t2amd_ffb_add_ln_bwd_f32")


def ffb_colsum(g, z, mean, rstd, lengths, dbias, dweight, ws):
    """dbias (C) = the column sums of g (B, T, C) over the real rows and, with z, mean and rstd, dweight (C) = those of
    g (z - mean) rstd; ``ws`` a uint8 tensor of at least ``fft_block_workspace(B, T, C, C, 1, 2)`` bytes."""
    who = "ffb_colsum"
    B, T, C_ = _ffb_shape(who, g, "g")
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_ffb_colsum_f32(_exact(who, g, "g", g.shape), _exact(who, z, "z", g.shape), _exact(who, mean, "mean", (B, T)),
                                       _exact(who, rstd, "rstd", (B, T)), _pair_lengths(who, lengths, B), B, T, C_,
                                       _exact(who, dbias, "dbias", (C_,)), _exact(who, dweight, "dweight", (C_,)), pw, nw, _stream()),
           "t2amd_ffb_colsum_f32")


def ffb_relu_mask(g, y, lengths, out):
    """out = g where y > 0 and +0 elsewhere and beyond ``lengths``: the gradient below a ReLU; all (B, T, C) contiguous."""
    who = "ffb_relu_mask"
    B, T, C_ = _ffb_shape(who, g, "g")
    _check(load().t2amd_ffb_relu_mask_f32(_exact(who, g, "g", g.shape), _exact(who, y, "y", g.shape), _pair_lengths(who, lengths, B),
                                          B, T, C_, _exact(who, out, "out", g.shape), _stream()), "t2amd_ffb_relu_mask_f32")


# ---- the thin ends of a temporal predictor: channel projection and scalar embedding (csrc/predictor_rows.hip) --------------------
def predictor_limits():
    """-> (frames at most, channels at most, kernel width at most, scalar tracks at most, utterances at most)."""
    return _query_ints("t2amd_predictor_limits", 5)


def predictor_workspace(B, T, C_, P, k, which):
    """Bytes for B utterances of at most T frames, C channels, P tracks and k taps: ``which`` 0 the forwards and the input
    gradients (none), 1 the projection's dw and db, 2 the embedding's."""
    return _query_bytes("t2amd_predictor_workspace", int(B), int(T), int(C_), int(P), int(k), int(which))


def _pred_shape(who, x, name, axes="(B, T, C)"):
    if x.dim() != 3:
        raise NativeError("%s: expected %s %s, got %s" % (who, name, axes, tuple(x.shape)))
    return x.shape


def pred_project(h, w, bias, lengths, y):
    """y (B, T, P) = bias + h w^T on the rows below ``lengths`` (device int32, clamped; None: T), +0 beyond; h (B, T, C), w (P, C),
    ``bias`` (P) or None; all contiguous."""
    who = "pred_project"
    B, T, C_ = _pred_shape(who, h, "h")
    P = w.shape[0] if w.dim() == 2 else -1
    _check(load().t2amd_pred_project_f32(_exact(who, h, "h", h.shape), _exact(who, w, "w", (P, C_)), _exact(who, bias, "bias", (P,)),
                                         _pair_lengths(who, lengths, B), B, T, C_, P, _exact(who, y, "y", (B, T, P)), _stream()),
           "t2amd_pred_project_f32")


def pred_project_backward(g, w, lengths, dh):
    """dh (B, T, C) = g w on the rows below ``lengths``, +0 beyond; g (B, T, P), w (P, C)."""
    who = "pred_project_backward"
    B, T, C_ = _pred_shape(who, dh, "dh")
    P = w.shape[0] if w.dim() == 2 else -1
    _check(load().t2amd_pred_project_bwd_f32(_exact(who, g, "g", (B, T, P)), _exact(who, w, "w", (P, C_)), _pair_lengths(who, lengths, B),
                                             B, T, C_, P, _exact(who, dh, "dh", dh.shape), _stream()), "t2amd_pred_project_bwd_f32")


def pred_project_sums(g, h, lengths, dw, db, ws):
    """dw (P, C) = the sum of g(b, t, p) h(b, t, c) and db (P) = the sum of g over the real rows (either may be None); ``ws`` a uint8
    tensor of at least ``predictor_workspace(B, T, C, P, 1, 1)`` bytes."""
    who = "pred_project_sums"
    B, T, C_ = _pred_shape(who, h, "h")
    P = g.shape[2] if g.dim() == 3 else -1
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_pred_project_sums_f32(_exact(who, g, "g", (B, T, P)), _exact(who, h, "h", h.shape), _pair_lengths(who, lengths, B),
                                              B, T, C_, P, _exact(who, dw, "dw", (P, C_)), _exact(who, db, "db", (P,)), pw, nw, _stream()),
           "t2amd_pred_project_sums_f32")


def pred_embed(v, image, bias, base, lengths, k, y):
    """y (B, T, C) = base + (bias + the k-tap embedding of the tracks v (B, T, P) under ``image`` (P k, C)), every utterance alone over
    its own ``lengths[b]`` frames, +0 at and beyond them; ``bias`` (C) and ``base`` (B, T, C) may be None."""
    who = "pred_embed"
    B, T, C_ = _pred_shape(who, y, "y")
    P = v.shape[2] if v.dim() == 3 else -1
    _check(load().t2amd_pred_embed_f32(_exact(who, v, "v", (B, T, P)), _exact(who, image, "the weight image", (P * int(k), C_)),
                                       _exact(who, bias, "bias", (C_,)), _exact(who, base, "base", y.shape),
                                       _pair_lengths(who, lengths, B), B, T, C_, P, int(k), _exact(who, y, "y", y.shape), _stream()),
           "t2amd_pred_embed_f32")


def pred_embed_backward(g, image, lengths, P, k, dbase, dv):
    """dbase (B, T, C) = g on the real rows and +0 beyond; dv (B, T, P) = the gradient of the tracks under ``image`` (P k, C);
    either may be None (``image`` too without dv)."""
    who = "pred_embed_backward"
    B, T, C_ = _pred_shape(who, g, "g")
    _check(load().t2amd_pred_embed_bwd_f32(_exact(who, g, "g", g.shape), _exact(who, image, "the weight image", (int(P) * int(k), C_)),
                                           _pair_lengths(who, lengths, B), B, T, C_, int(P), int(k), _exact(who, dbase, "dbase", g.shape),
                                           _exact(who, dv, "dv", (B, T, int(P))), _stream()), "t2amd_pred_embed_bwd_f32")


def pred_embed_sums(g, v, lengths, k, dw, db, ws):
    """dw (C, P, k) = the sum of g(b, t, c) v(b, t + j - k // 2, p) and db (C) = the sum of g over the real rows (either may be None);
    ``ws`` a uint8 tensor of at least ``predictor_workspace(B, T, C, P, k, 2)`` bytes."""
    who = "pred_embed_sums"
    B, T, C_ = _pred_shape(who, g, "g")
    P = v.shape[2] if v.dim() == 3 else -1
    pw, nw = _workspace(who, ws)
    _check(load().t2amd_pred_embed_sums_f32(_exact(who, g, "g", g.shape), _exact(who, v, "v", (B, T, P)), _pair_lengths(who, lengths, B),
                                            B, T, C_, P, int(k), _exact(who, dw, "dw", (C_, P, int(k))), _exact(who, db, "db", (C_,)),
                                            pw, nw, _stream()), "t2amd_pred_embed_sums_f32")


# ----------------------------------------------------------------------------
# Griffin-Lim vocoder (csrc/vocoder.hip)
# ----------------------------------------------------------------------------
def _host_ints(values):
    """Host int32 array of the lengths (passed through when it already is one: the Griffin-Lim loop builds it once)."""
    if isinstance(values, C.Array):
        return values
    vals = [int(v) for v in values]
    if not vals:
        raise NativeError("empty length list")
    return (C.c_int * len(vals))(*vals)


def gl_packed_rows(lengths, L, hop):
    """sum(n_b + ceil(L/hop) - 1): rows of the packed frame space (-1 for bad arguments)."""
    n = _host_ints(lengths)
    return int(load().t2amd_gl_packed_rows(n, len(n), int(L), int(hop)))


def gl_overlap_add(frames, wsq, plan, lengths, R, L, hop, scale, out, mode, out_len=None):
    """mode 0: out (1-D, packed reflect-padded signal); mode 1: out (B, T) trimmed signal (zero beyond each T_b)."""
    pf, ldf, _, _ = _mat(frames)
    n = _host_ints(lengths)
    if mode == 0:
        po, ldo, olen = ptr(_fullc(out)), 0, out.numel() if out_len is None else out_len
    else:
        po, ldo, _, olen = _mat(out)
    _check(load().t2amd_gl_overlap_add_f32(pf, _i64(ldf), ptr(wsq, torch.float64), ptr(plan, torch.int32), n,
                                           len(n), _i64(R), int(L), int(hop), C.c_float(scale), po, _i64(ldo), _i64(olen),
                                           int(mode), _stream()), "t2amd_gl_overlap_add_f32")


def gl_project(spec, S, plan, lengths, R, L, hop, F, Fp, rec):
    ps, lds, _, _ = _mat(spec)
    pS, ldS, _, _ = _mat(S)
    pr, ldr, _, _ = _mat(rec)
    n = _host_ints(lengths)
    _check(load().t2amd_gl_project_f32(ps, _i64(lds), pS, _i64(ldS), ptr(plan, torch.int32), n, len(n), _i64(R),
                                       int(L), int(hop), int(F), int(Fp), pr, _i64(ldr), _stream()), "t2amd_gl_project_f32")


def gl_rect(mag, phase, plan, lengths, R, L, hop, F, Fp, S, rec):
    """mag/phase (B, F, n) contiguous (phase None: 0; mag None: magnitudes already in S)."""
    src = mag if mag is not None else phase
    ldn = src.shape[-1] if src is not None else 0
    pS, ldS, _, _ = _mat(S)
    pr, ldr, _, _ = _mat(rec)
    n = _host_ints(lengths)
    _check(load().t2amd_gl_rect_f32(ptr(_fullc(mag)) if mag is not None else None,
                                    ptr(_fullc(phase)) if phase is not None else None, _i64(ldn), ptr(plan, torch.int32),
                                    n, len(n), _i64(R), int(L), int(hop), int(F), int(Fp), pS, _i64(ldS), pr,
                                    _i64(ldr), _stream()), "t2amd_gl_rect_f32")


def stft_polar(spec, B, n, F, mag, phase):
    """spec rows (B*n, interleaved re/im) -> mag, phase (B, F, n)."""
    ps, lds, R, _ = _mat(spec)
    if R != B * n:
        raise NativeError("stft_polar: %d spectrum rows for B=%d, n=%d" % (R, B, n))
    _check(load().t2amd_stft_polar_f32(ps, _i64(lds), int(B), int(n), int(F),
                                       ptr(_fullc(mag)) if mag is not None else None,
                                       ptr(_fullc(phase)) if phase is not None else None, _stream()), "t2amd_stft_polar_f32")


def mel_decompress(mel, out, lengths=None, lengths_dev=None):
    """out (B*n, ld) = exp(mel (B, n_mel, n)) transposed, zero beyond lengths and n_mel."""
    B, n_mel, n = mel.shape
    po, ld, R, _ = _mat(out)
    if R != B * n:
        raise NativeError("mel_decompress: shape mismatch mel=%s out=%s" % (tuple(mel.shape), tuple(out.shape)))
    nh = _host_ints(lengths) if lengths is not None else None
    _check(load().t2amd_mel_decompress_f32(ptr(_fullc(mel)), B, n_mel, n,
                                           ptr(lengths_dev, torch.int32) if lengths_dev is not None else None, nh, po,
                                           _i64(ld), _stream()), "t2amd_mel_decompress_f32")


# ----------------------------------------------------------------------------
# WaveGlow (csrc/waveglow.hip, csrc/waveglow_layer.hip)
# ----------------------------------------------------------------------------
def _opt(t, dtype=torch.float32):
    return ptr(_fullc(t), dtype) if t is not None else None


def wg_gated(X, W, bias, dil, cnd, acts, precision, gate=None):
    """acts[m][0:C] = tanh * sigmoid of the dilated kernel-3 product of the halo image X (a view whose rows continue
    for at least `dil` rows on both sides) with the gate-packed weights W [2C][3C] (+ bias, + cnd[m][0:2C]).
    gate [M][2C] (the training forward): the tanh values and the sigmoid values, in channel order, kept for the backward pass."""
    px, ldx, M, Cin = _mat(X)
    pw, _, N, K = _mat(W)
    pc, ldc, Mc, Nc = _mat(cnd)
    pa, lda, Ma, Ca = _mat(acts)
    if K != 3 * Cin or Mc != M or Ma != M or Nc != N or 2 * Ca != N or bias.numel() != N:
        raise NativeError("wg_gated: shape mismatch X=%s W=%s cnd=%s acts=%s" % (tuple(X.shape), tuple(W.shape),
                                                                                tuple(cnd.shape), tuple(acts.shape)))
    if gate is not None:
        pg, ldg, Mg, Ng = _mat(gate)
        if Mg != M or Ng != N:
            raise NativeError("wg_gated: gate %s for %d rows of %d values" % (tuple(gate.shape), M, N))
        _check(load().t2amd_wg_layer_train_f32(px, _i64(ldx), pw, ptr(_fullc(bias)), M, N, Cin, 3, int(dil), 0, pc, _i64(ldc),
                                               pa, _i64(lda), None, 0, 0, None, 0, 0, None, pg, _i64(ldg), None, 0,
                                               int(precision), _stream()), "t2amd_wg_layer_train_f32")
        return
    _check(load().t2amd_wg_layer_f32(px, _i64(ldx), pw, ptr(_fullc(bias)), M, N, Cin, 3, int(dil), 0, pc, _i64(ldc), pa,
                                     _i64(lda), None, 0, 0, None, 0, 0, None, int(precision), _stream()),
           "t2amd_wg_layer_f32")


def wg_res_skip(acts, W, bias, h, skip, skip_store, rowb, precision, h_out=None):
    """h[m] += (acts . W^T + bias)[0:C] on rows with rowb >= 0 (h None: the last layer, no residual half);
    skip[m] (+)= the remaining columns.  h_out (the training forward): h_out[m] = h[m] + ... instead, h is left as it is."""
    px, ldx, M, Cin = _mat(acts)
    pw, _, N, K = _mat(W)
    ps, lds, Ms, Cs = _mat(skip)
    nres = 0
    ph, ldh = None, 0
    if h is not None:
        ph, ldh, Mh, nres = _mat(h)
        if Mh != M:
            raise NativeError("wg_res_skip: h rows")
    if K != Cin or Ms != M or N - nres != Cs or bias.numel() != N or rowb.numel() < M:
        raise NativeError("wg_res_skip: shape mismatch acts=%s W=%s skip=%s" % (tuple(acts.shape), tuple(W.shape),
                                                                               tuple(skip.shape)))
    if h_out is not None:
        if h is None:
            raise NativeError("wg_res_skip: h_out without h")
        po, ldo, Mo, No = _mat(h_out)
        if Mo != M or No != nres:
            raise NativeError("wg_res_skip: h_out %s beside h %s" % (tuple(h_out.shape), tuple(h.shape)))
        _check(load().t2amd_wg_layer_train_f32(px, _i64(ldx), pw, ptr(_fullc(bias)), M, N, Cin, 1, 1, 1, None, 0, None, 0, ph,
                                               _i64(ldh), nres, ps, _i64(lds), 1 if skip_store else 0,
                                               ptr(rowb, torch.int32), None, 0, po, _i64(ldo), int(precision), _stream()),
               "t2amd_wg_layer_train_f32")
        return
    _check(load().t2amd_wg_layer_f32(px, _i64(ldx), pw, ptr(_fullc(bias)), M, N, Cin, 1, 1, 1, None, 0, None, 0, ph,
                                     _i64(ldh), nres, ps, _i64(lds), 1 if skip_store else 0, ptr(rowb, torch.int32),
                                     int(precision), _stream()), "t2amd_wg_layer_f32")


def wg_dgrad(d_pre, Wt, dil, dh, store, rowb, precision):
    """The in-layer product's data gradient in one launch: dh[m] (+)= sum over the three taps of d_pre[m -+ dil] . W on rows
    with rowb >= 0 (``store``: plain store).  d_pre [M][2C] is a view whose rows continue, zero, for at least `dil` rows on
    both sides; Wt [C][3 * 2C] holds the transposed weights with the taps mirrored (WaveGlow._packed's ``in_wT``)."""
    px, ldx, M, Cin = _mat(d_pre)
    pw, _, N, K = _mat(Wt)
    ph, ldh, Mh, Nh = _mat(dh)
    if K != 3 * Cin or Mh != M or Nh != N or rowb.numel() < M:
        raise NativeError("wg_dgrad: shape mismatch d_pre=%s Wt=%s dh=%s" % (tuple(d_pre.shape), tuple(Wt.shape),
                                                                            tuple(dh.shape)))
    _fullc(Wt)
    _check(load().t2amd_wg_layer_train_f32(px, _i64(ldx), pw, None, M, N, Cin, 3, int(dil), 2, None, 0, None, 0, ph, _i64(ldh),
                                           0, None, 0, 1 if store else 0, ptr(rowb, torch.int32), None, 0, None, 0,
                                           int(precision), _stream()), "t2amd_wg_layer_train_f32")


def wg_tail(rowb, rowr, audio, n_group, skip=None, end_w=None, end_b=None, winv=None, z=None, sigma=0.0,
            start_w=None, start_b=None, h=None, out=None):
    """The flow tail over every packed row (see the header).  z: the (B, n_new, R) noise tensor (contiguous);
    start_w (C, n_half') and end_w (n_in, C) contiguous; out (B, >= n_group R) waveform rows."""
    P = rowb.numel()
    pa, lda, Pa, _ = _mat(audio)
    if Pa != P or rowr.numel() != P:
        raise NativeError("wg_tail: %d audio rows / %d rowr for %d packed rows" % (Pa, rowr.numel(), P))
    n_in, nc = (end_w.shape[0], end_w.shape[1]) if end_w is not None else (0, 0)
    ps, lds = None, 0
    if skip is not None:
        ps, lds, _, cs = _mat(skip)
        nc = nc or cs
    if start_w is not None:
        nc = nc or start_w.shape[0]
    ph, ldh = None, 0
    if h is not None:
        ph, ldh, _, _ = _mat(h)
    zp, zb, zc, n_new = None, 0, 0, 0
    if z is not None:
        _fullc(z)
        zp, zb, zc, n_new = ptr(z), z.stride(0), z.stride(1), z.shape[1]
    po, ldo = None, 0
    if out is not None:
        po, ldo, _, _ = _mat(out)
    _check(load().t2amd_wg_tail_f32(ps, _i64(lds), int(nc), _opt(end_w), _opt(end_b), int(n_in), _opt(winv), pa, _i64(lda),
                                    zp, _i64(zb), _i64(zc), int(n_new), _F(sigma),
                                    _opt(start_w), _opt(start_b), ph, _i64(ldh), po, _i64(ldo), ptr(rowb, torch.int32),
                                    ptr(rowr, torch.int32), _i64(P), int(n_group), _stream()), "t2amd_wg_tail_f32")


def wg_denoise(mag, bias, strength):
    """mag (B, F, n) = max(mag - bias (F,) * strength, 0), in place."""
    B, F, n = mag.shape
    if bias.numel() != F:
        raise NativeError("wg_denoise: bias has %d entries for %d bins" % (bias.numel(), F))
    _check(load().t2amd_wg_denoise_f32(ptr(_fullc(mag)), ptr(_fullc(bias)), B, F, _i64(n), _F(strength), _stream()),
           "t2amd_wg_denoise_f32")


# ----------------------------------------------------------------------------
# WaveGlow forward direction (csrc/waveglow_fwd.hip)
# ----------------------------------------------------------------------------
def _chan_rows(t, what, dtype=torch.float32):
    """(B, c, R) tensor with unit row stride -> (ptr, batch stride, channel stride, c, R)."""
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise NativeError("%s: expected a (B, channels, rows) tensor with contiguous rows, got shape %s stride %s"
                          % (what, tuple(t.shape), t.stride()))
    return ptr(t, dtype), t.stride(0), t.stride(1), t.shape[1], t.shape[2]


def wg_head(rowb, rowr, audio, n_group, B, R, skip=None, end_w=None, end_b=None, log_s=None, wave=None, z=None, z_off=0,
            n_emit=0, mix_w=None, start_w=None, start_b=None, h=None, save=None):
    """The flow head over every packed row (see the header).  save [P][2 n_group] (the training forward) keeps the rows
    before and after the mix.  log_s (B, n_in / 2, R) and z (B, n_group, R) with contiguous
    rows (any batch / channel stride); wave (B, >= n_group R) waveform rows; end_w (n_in, C), mix_w (n_out, n_out) and
    start_w (C, n_out / 2) contiguous."""
    P = rowb.numel()
    pa, lda, Pa, _ = _mat(audio)
    if Pa != P or rowr.numel() != P:
        raise NativeError("wg_head: %d audio rows / %d rowr for %d packed rows" % (Pa, rowr.numel(), P))
    n_in, nc = (end_w.shape[0], end_w.shape[1]) if end_w is not None else (0, 0)
    ps, lds = None, 0
    if skip is not None:
        ps, lds, _, cs = _mat(skip)
        nc = nc or cs
    if start_w is not None:
        nc = nc or start_w.shape[0]
    ph, ldh = None, 0
    if h is not None:
        ph, ldh, _, ch = _mat(h)
        nc = nc or ch
    pl, lsb, lsc = None, 0, 0
    if log_s is not None:
        pl, lsb, lsc, nl, Rl = _chan_rows(log_s, "wg_head: log_s")
        if (nl, Rl, log_s.shape[0]) != (n_in // 2, R, B):
            raise NativeError("wg_head: log_s %s for B=%d, n_in=%d, R=%d" % (tuple(log_s.shape), B, n_in, R))
    pz, zb, zc = None, 0, 0
    if z is not None:
        pz, zb, zc, nz, Rz = _chan_rows(z, "wg_head: z")
        if (nz, Rz, z.shape[0]) != (n_group, R, B):
            raise NativeError("wg_head: z %s for B=%d, n_group=%d, R=%d" % (tuple(z.shape), B, n_group, R))
    pw, ldw = None, 0
    if wave is not None:
        pw, ldw, Bw, _ = _mat(wave)
        if Bw != B:
            raise NativeError("wg_head: %d waveforms for B=%d" % (Bw, B))
    if mix_w is not None and (mix_w.dim() != 2 or mix_w.shape[0] != mix_w.shape[1] or start_w is None
                              or start_w.dim() != 2 or 2 * start_w.shape[1] != mix_w.shape[0]):
        raise NativeError("wg_head: mix_w (n, n) needs start_w (C, n / 2)")
    if save is not None:
        psv, ldsv, Psv, nsv = _mat(save)
        if Psv != P or nsv != 2 * n_group:
            raise NativeError("wg_head: save %s for %d packed rows of 2 x %d values" % (tuple(save.shape), P, n_group))
        _check(load().t2amd_wg_head_save_f32(ps, _i64(lds), int(nc), _opt(end_w), _opt(end_b), int(n_in), pl, _i64(lsb),
                                             _i64(lsc), pw, _i64(ldw), pa, _i64(lda), pz, _i64(zb), _i64(zc), int(z_off),
                                             int(n_emit), _opt(mix_w), _opt(start_w), _opt(start_b), ph, _i64(ldh),
                                             ptr(rowb, torch.int32), ptr(rowr, torch.int32), _i64(P), int(n_group), int(B),
                                             _i64(R), psv, _i64(ldsv), _stream()), "t2amd_wg_head_save_f32")
        return
    _check(load().t2amd_wg_head_f32(ps, _i64(lds), int(nc), _opt(end_w), _opt(end_b), int(n_in), pl, _i64(lsb), _i64(lsc),
                                    pw, _i64(ldw), pa, _i64(lda), pz, _i64(zb), _i64(zc), int(z_off), int(n_emit),
                                    _opt(mix_w), _opt(start_w), _opt(start_b), ph, _i64(ldh), ptr(rowb, torch.int32),
                                    ptr(rowr, torch.int32), _i64(P), int(n_group), int(B), _i64(R), _stream()),
           "t2amd_wg_head_f32")


def wg_nll_chunk():
    return int(load().t2amd_wg_nll_chunk())


def wg_nll(z, log_s, rows, partial, out):
    """out (B, 2) float64 = per utterance {sum z^2, sum log_s} over the first rows[b] (device int32) rows of z (B, c, R) and
    log_s (B, c', R) (None: 0), rows contiguous.  partial: float64 workspace, >= B * ceil(R / wg_nll_chunk()) * 2."""
    pz, zb, zc, nz, R = _chan_rows(z, "wg_nll: z")
    B = z.shape[0]
    pl, lb, lc, nls = None, 0, 0, 0
    if log_s is not None:
        pl, lb, lc, nls, Rl = _chan_rows(log_s, "wg_nll: log_s")
        if Rl != R or log_s.shape[0] != B:
            raise NativeError("wg_nll: log_s %s beside z %s" % (tuple(log_s.shape), tuple(z.shape)))
    nchunk = (R + wg_nll_chunk() - 1) // wg_nll_chunk()
    if rows.numel() != B or partial.numel() < B * nchunk * 2 or out.numel() != 2 * B:
        raise NativeError("wg_nll: %d row counts, %d partials, %d outputs for B=%d, R=%d" % (rows.numel(), partial.numel(),
                                                                                           out.numel(), B, R))
    _check(load().t2amd_wg_nll_f32(pz, _i64(zb), _i64(zc), int(nz), pl, _i64(lb), _i64(lc), int(nls), ptr(rows, torch.int32),
                                   int(B), _i64(R), ptr(_fullc(partial), torch.float64), _i64(nchunk),
                                   ptr(_fullc(out), torch.float64), _stream()), "t2amd_wg_nll_f32")


# ----------------------------------------------------------------------------
# WaveGlow backward pass (csrc/waveglow_bwd.hip)
# ----------------------------------------------------------------------------
def wg_head_bwd_rows():
    return int(load().t2amd_wg_head_bwd_rows())


def wg_head_bwd_sizes(C, n_in, n_out):
    """Number of small gradients one head call produces: [end_w | end_b] (n_in > 0) + [start_w | start_b | mix] (n_out > 0)."""
    n = n_in * C + n_in if n_in else 0
    return n + (C * (n_out // 2) + C + n_out * n_out if n_out else 0)


def wg_head_bwd(rowb, rowr, n_group, B, R, c1, c2, x_sv, partial, n_emit=0, skip=None, end_w=None, log_s=None, a_in=None,
                dA=None, d_skip=None, dh0=None, mix_w=None, start_w=None, a_sv=None):
    """Backward of one flow head call (see the header) -> (workgroups, small gradients per workgroup): ``partial`` holds the
    per-workgroup partial sums for ``wg_partial_sum``.  x_sv / a_sv: the rows the call kept; a_in: the a rows of the call
    before; dA [P][>= n_group] in / out; dh0 [P][C]; d_skip [P][C] out."""
    P = rowb.numel()
    if rowr.numel() != P:
        raise NativeError("wg_head_bwd: %d rowr for %d packed rows" % (rowr.numel(), P))

    def rows(t, what):
        if t is None:
            return None, 0, 0
        p_, ld, Pt, n = _mat(t)
        if Pt != P:
            raise NativeError("wg_head_bwd: %s has %d rows for %d packed rows" % (what, Pt, P))
        return p_, ld, n

    n_in, C = (end_w.shape[0], end_w.shape[1]) if end_w is not None else (0, 0)
    if start_w is not None:
        C = C or start_w.shape[0]
    n_cur = n_in if end_w is not None else n_group
    n_out = n_cur - n_emit if mix_w is not None else 0
    if mix_w is not None and (mix_w.dim() != 2 or tuple(mix_w.shape) != (n_out, n_out) or start_w is None
                              or start_w.dim() != 2 or tuple(start_w.shape) != (C, n_out // 2)):
        raise NativeError("wg_head_bwd: mix_w (n_out, n_out) needs start_w (C, n_out / 2), n_out = %d" % n_out)
    ps, lds, _ = rows(skip, "skip")
    pai, ldai, _ = rows(a_in, "a_in")
    px, ldx, _ = rows(x_sv, "x_sv")
    pas, ldas, _ = rows(a_sv, "a_sv")
    pdA, lddA, _ = rows(dA, "dA")
    pdh, lddh, _ = rows(dh0, "dh0")
    pds, ldds, _ = rows(d_skip, "d_skip")
    pl, lsb, lsc = None, 0, 0
    if log_s is not None:
        pl, lsb, lsc, nl, Rl = _chan_rows(log_s, "wg_head_bwd: log_s")
        if (nl, Rl, log_s.shape[0]) != (n_in // 2, R, B):
            raise NativeError("wg_head_bwd: log_s %s for B=%d, n_in=%d, R=%d" % (tuple(log_s.shape), B, n_in, R))
    npart = wg_head_bwd_sizes(C, n_in, n_out)
    nblk = -(-P // wg_head_bwd_rows())
    if partial.numel() < nblk * npart:
        raise NativeError("wg_head_bwd: partial holds %d values, %d workgroups x %d needed" % (partial.numel(), nblk, npart))
    _check(load().t2amd_wg_head_bwd_f32(ps, _i64(lds), int(C), _opt(end_w), int(n_in), pl, _i64(lsb), _i64(lsc), pai, _i64(ldai),
                                        px, _i64(ldx), pas, _i64(ldas), pdA, _i64(lddA), pdh, _i64(lddh), _opt(mix_w),
                                        _opt(start_w), int(n_emit), pds, _i64(ldds), ptr(_fullc(partial)), _i64(npart),
                                        ptr(rowb, torch.int32), ptr(rowr, torch.int32), _i64(P), int(n_group), int(B), _i64(R),
                                        _F(c1), _F(c2), _stream()), "t2amd_wg_head_bwd_f32")
    return nblk, npart


def wg_partial_sum(partial, nblk, n, out):
    """out[0:n] = sum over the first nblk blocks of n values of ``partial``, in block order."""
    if partial.numel() < nblk * n or out.numel() != n:
        raise NativeError("wg_partial_sum: %d partials, %d outputs for %d blocks of %d" % (partial.numel(), out.numel(), nblk, n))
    _check(load().t2amd_wg_partial_sum_f32(ptr(_fullc(partial)), _i64(nblk), _i64(n), ptr(_fullc(out)), _stream()),
           "t2amd_wg_partial_sum_f32")


def wg_gate_bwd(d_acts, gate, rowb, d_pre, acts):
    """d_pre [M][2C] and acts [M][C] from d_acts [M][C] and the kept gate values gate [M][2C], on rows with rowb >= 0."""
    pd, ldd, M, Cc = _mat(d_acts)
    pg, ldg, Mg, Ng = _mat(gate)
    pp, ldp, Mp, Np = _mat(d_pre)
    pa, lda, Ma, Na = _mat(acts)
    if (Mg, Mp, Ma) != (M, M, M) or (Ng, Np, Na) != (2 * Cc, 2 * Cc, Cc) or rowb.numel() < M:
        raise NativeError("wg_gate_bwd: shape mismatch d_acts=%s gate=%s d_pre=%s acts=%s"
                          % (tuple(d_acts.shape), tuple(gate.shape), tuple(d_pre.shape), tuple(acts.shape)))
    _check(load().t2amd_wg_gate_bwd_f32(pd, _i64(ldd), pg, _i64(ldg), ptr(rowb, torch.int32), _i64(M), int(Cc), pp, _i64(ldp),
                                        pa, _i64(lda), _stream()), "t2amd_wg_gate_bwd_f32")


WG_WN_SHORT = 4        # rows of at most this many floats are folded one per lane, 64 per work unit (WGN_SHORT of the kernels)


def wg_weight_norm_table(segments):
    """-> (int64 [n][6] host table, work units) for ``segments`` = [(off, goff, dwoff, rows, len)]: the layout
    t2amd_wg_weight_norm_f32 reads (include/tacotron2_amd.h), the work units counted through the table."""
    short = WG_WN_SHORT
    lines, first = [], 0
    for off, goff, dwoff, rows, ln in segments:
        lines.append([int(off), int(goff), int(dwoff), int(rows), int(ln), first])
        first += -(-int(rows) // 64) if ln <= short else int(rows)
    return torch.tensor(lines, dtype=torch.int64).view(-1, 6), first


def _wn_table_check(who, table, host, n_units, big, small, dw=None):
    """The kernels trust the table: every line is checked here, on the host copy, against the buffers it addresses."""
    if host.dtype != torch.int64 or host.dim() != 2 or host.shape[1] != 6 or host.shape[0] < 1 or host.is_cuda:
        raise NativeError("%s: the host table must be an int64 [n][6] CPU tensor" % who)
    if table.dtype != torch.int64 or tuple(table.shape) != tuple(host.shape) or not table.is_contiguous():
        raise NativeError("%s: the device table must be a contiguous int64 tensor of the host table's shape" % who)
    short = WG_WN_SHORT
    if int(load().t2amd_wg_weight_norm_short()) != short:
        raise NativeError("%s: the library folds rows of up to %d floats per lane, native.py expects %d"
                          % (who, load().t2amd_wg_weight_norm_short(), short))
    first = 0
    for s, (off, goff, dwoff, rows, ln, f) in enumerate(host.tolist()):
        if rows < 1 or ln < 1 or off < 0 or goff < 0 or dwoff < 0:
            raise NativeError("%s: table line %d: bad rows / len / offsets" % (who, s))
        if f != first:
            raise NativeError("%s: table line %d starts at work unit %d, expected %d" % (who, s, f, first))
        first += -(-rows // 64) if ln <= short else rows
        if ln > short and ln % 4 == 0 and (off % 4 or (dw is not None and dwoff % 4)):
            raise NativeError("%s: table line %d: rows of a multiple of 4 floats must start at a multiple of 4 floats"
                              % (who, s))
        for t in big:
            if off + rows * ln > t.numel():
                raise NativeError("%s: table line %d reaches float %d of a buffer of %d" % (who, s, off + rows * ln, t.numel()))
        for t in small:
            if goff + rows > t.numel():
                raise NativeError("%s: table line %d reaches row %d of a buffer of %d" % (who, s, goff + rows, t.numel()))
        if dw is not None and dwoff + rows * ln > dw.numel():
            raise NativeError("%s: table line %d reaches float %d of a gradient buffer of %d"
                              % (who, s, dwoff + rows * ln, dw.numel()))
    if first != n_units:
        raise NativeError("%s: the table holds %d work units, not %d" % (who, first, n_units))
    for t in list(big) + list(small) + ([dw] if dw is not None else []):
        if t.dim() != 1:
            raise NativeError("%s: the buffers are flat (1-D) tensors" % who)
        _fullc(t)


def wg_weight_norm(table, host, n_units, v, g, w, norm):
    """The fold of every tensor of the table in one launch: w = v g / ||v|| per row, norm = ||v|| (flat f32 buffers;
    ``table`` on the device, ``host`` its CPU copy, both from ``wg_weight_norm_table``)."""
    _wn_table_check("wg_weight_norm", table, host, n_units, (v, w), (g, norm))
    _check(load().t2amd_wg_weight_norm_f32(ptr(table, torch.int64), int(host.shape[0]), _i64(n_units), ptr(v), ptr(g), ptr(w),
                                           ptr(norm), _stream()), "t2amd_wg_weight_norm_f32")


def wg_weight_norm_bwd(table, host, n_units, dw, v, g, norm, dg, dv, scale=1.0):
    """The fold's backward in one launch: dg, dv (laid out like g, v) from dw (at the table's dwoff), times ``scale``."""
    _wn_table_check("wg_weight_norm_bwd", table, host, n_units, (v, dv), (g, norm, dg), dw=dw)
    _check(load().t2amd_wg_weight_norm_bwd_f32(ptr(table, torch.int64), int(host.shape[0]), _i64(n_units), ptr(dw), ptr(v),
                                               ptr(g), ptr(norm), ptr(dg), ptr(dv), _F(float(scale)), _stream()),
           "t2amd_wg_weight_norm_bwd_f32")


# ----------------------------------------------------------------------------
# HiFi-GAN generator (csrc/hifigan.hip, csrc/hifigan_post.hip)
# ----------------------------------------------------------------------------
def _floats(t):
    """Elements of t's storage from t's first element on: what the hg_* entries check the addressed rows against."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _image(t, out=False):
    """A row image [P][C] -> (its arguments as the hg_* / vc_* entries take them, P, C): an operand is (pointer, addressed
    floats, row stride, rows, width), an output or a residual (pointer, row stride, addressed floats).  The entries take
    them in this order; one that takes no width (vc_polar, vc_ola) gets the operand's first four, ``[:4]``."""
    p, ld, P, C = _mat(t)
    return ((p, ld, _floats(t)) if out else (p, _floats(t), ld, P, C)), P, C


def _res(who, res, out):
    """The arguments of the optional residual image beside out; a null image without one."""
    if res is None:
        return None, 0, 0                            # the triple of _image(res, True) for no image
    r, Pr, Nr = _image(res, True)
    if (Pr, Nr) != tuple(out.shape):
        raise NativeError("%s: res %s beside out %s" % (who, tuple(res.shape), tuple(out.shape)))
    return r


def _vec(t):
    """An optional contiguous float32 vector -> pointer or NULL."""
    return None if t is None else ptr(_fullc(t))


def _hg_map(rowb0, rowr0=None):
    """The row map -> (rowb0's pointer, [rowr0's pointer,] map rows)."""
    if rowb0.dtype != torch.int32 or rowb0.dim() != 1 or not rowb0.is_contiguous():
        raise NativeError("hifigan: rowb0 must be a contiguous int32 vector")
    if rowr0 is not None and (rowr0.dtype != torch.int32 or rowr0.shape != rowb0.shape or not rowr0.is_contiguous()):
        raise NativeError("hifigan: rowr0 must be an int32 vector of rowb0's length")
    return (ptr(rowb0, torch.int32),) + (() if rowr0 is None else (ptr(rowr0, torch.int32),)) + (rowb0.numel(),)


def hg_conv(X, W, bias, taps, dil, slope, res, out, scale, accumulate, rowb0, rdiv, precision):
    """out [P][N] = epi(bias + the dilated `taps`-tap product of the row image X [P][Cin] with W [N][taps * Cin]), leaky-ReLU
    (`slope`; None: none) on the operand; epi: (+ res) * scale, stored or added into out; zero on rows whose frame-level row
    rowb0[p // rdiv] is negative."""
    x, P, Cin = _image(X)
    pw, ldw, N, K = _mat(W)
    o, Po, No = _image(out, True)
    if K != taps * Cin or ldw != K or Po != P or No != N or (bias is not None and bias.numel() != N):
        raise NativeError("hg_conv: shape mismatch X=%s W=%s out=%s taps=%d" % (tuple(X.shape), tuple(W.shape),
                                                                                  tuple(out.shape), taps))
    r, m = _res("hg_conv", res, out), _hg_map(rowb0)
    _check(load().t2amd_hg_conv_f32(*x, pw, _floats(W), _vec(bias), N, int(taps), int(dil), 0 if slope is None else 1,
                                    _F(0.0 if slope is None else slope), *r, *o, _F(scale), 1 if accumulate else 0,
                                    *m, int(rdiv), int(precision), _stream()), "t2amd_hg_conv_f32")


def hg_upsample(X, W, bias, ku, u, slope, out, rowb0, rdiv, precision):
    """out [u P][N] = ConvTranspose1d(kernel ku, stride u, padding (ku - u) / 2) of the row image X [P][Cin] as u polyphase
    products; W [u][N][(ku / u) * Cin] the per-phase weight slices (Generator._packed).  rdiv: that of X's rows."""
    x, P, Cin = _image(X)
    o, Po, N = _image(out, True)
    if W.dim() != 3 or not W.is_contiguous() or u < 1 or ku % u or tuple(W.shape) != (u, N, ku // u * Cin) or Po != u * P \
            or (bias is not None and bias.numel() != N):
        raise NativeError("hg_upsample: shape mismatch X=%s W=%s out=%s ku=%d u=%d" % (tuple(X.shape), tuple(W.shape),
                                                                                        tuple(out.shape), ku, u))
    _check(load().t2amd_hg_upsample_f32(*x, ptr(W), _floats(W), _vec(bias), N, int(ku), int(u), 0 if slope is None else 1,
                                        _F(0.0 if slope is None else slope), *o, *_hg_map(rowb0), int(rdiv),
                                        int(precision), _stream()), "t2amd_hg_upsample_f32")


def hg_post(X, w, bias, slope, rowb0, rowr0, rdiv, out):
    """conv_post: out (B, 1, T)[b, 0, rowr0[f] * rdiv + p % rdiv] = tanh(bias + 7-tap product of lrelu(X [P][C]) with w [7][C])
    for the rows p of real frames f = p // rdiv."""
    x, _, C = _image(X)
    if w.dim() != 2 or not w.is_contiguous() or w.shape[1] != C or bias.numel() != 1 or out.dim() != 3 or out.shape[1] != 1:
        raise NativeError("hg_post: shape mismatch X=%s w=%s out=%s" % (tuple(X.shape), tuple(w.shape), tuple(out.shape)))
    _check(load().t2amd_hg_post_f32(*x, ptr(w), w.numel(), ptr(bias), _F(slope), *_hg_map(rowb0, rowr0), int(rdiv),
                                    ptr(_fullc(out)), out.shape[2], out.numel(), _stream()), "t2amd_hg_post_f32")


def hg_pack_mel(mel, rowb0, rowr0, out):
    """out [P0][ldo] = the (B, n_mel, N) mels as frame-level rows: out[f][c] = mel[rowb0[f]][c][rowr0[f]], zero on halo
    rows and on the padding columns c >= n_mel."""
    o, P0, No = _image(out, True)
    if mel.dim() != 3 or No != o[1] or mel.shape[1] > No:
        raise NativeError("hg_pack_mel: mel %s into contiguous rows %s" % (tuple(mel.shape), tuple(out.shape)))
    m = _hg_map(rowb0, rowr0)
    if m[2] != P0:
        raise NativeError("hg_pack_mel: %d map rows for %d image rows" % (rowb0.numel(), P0))
    B, n_mel, N = mel.shape
    _check(load().t2amd_hg_pack_mel_f32(ptr(_fullc(mel)), _floats(mel), B, n_mel, N, *m, *o, _stream()),
           "t2amd_hg_pack_mel_f32")


# ----------------------------------------------------------------------------
# Vocos vocoder (csrc/vocos.hip, csrc/vocos_rows.hip)
# ----------------------------------------------------------------------------
VC_EPI = {None: 0, 'gelu': 1, 'residual': 2}


def vc_dwln(X, w, conv_bias, ln_w, ln_b, eps, rowb0, out):
    """out [P][D] = LayerNorm_D(conv_bias + the depthwise product of the row image X [P][D] with w [taps][D]) * ln_w + ln_b;
    w None: LayerNorm of X alone.  Zero on rows whose rowb0 is negative."""
    x, P, D = _image(X)
    o, Po, Do = _image(out, True)
    taps = 0 if w is None else int(w.shape[0])
    if (Po, Do) != (P, D) or ln_w.numel() != D or ln_b.numel() != D or \
            (w is not None and (w.dim() != 2 or w.shape[1] != D or conv_bias is None or conv_bias.numel() != D)):
        raise NativeError("vc_dwln: shape mismatch X=%s w=%s out=%s" % (tuple(X.shape), None if w is None else tuple(w.shape),
                                                                        tuple(out.shape)))
    _check(load().t2amd_vc_dwln_f32(*x, _vec(w), 0 if w is None else w.numel(), _vec(conv_bias) if w is not None else None,
                                    taps, _vec(ln_w), _vec(ln_b), _F(eps), *_hg_map(rowb0), *o, _stream()),
           "t2amd_vc_dwln_f32")


def vc_linear(X, W, bias, epi, gamma, res, out, rowb0, precision):
    """out [P][N] = epi(bias + X [P][K] W [N][K]^T); epi None, 'gelu' (exact) or 'residual' (res + gamma * .; res may be
    out).  Zero on rows whose rowb0 is negative."""
    x, P, K = _image(X)
    pw, ldw, N, Kw = _mat(W)
    o, Po, No = _image(out, True)
    if epi not in VC_EPI:
        raise NativeError("vc_linear: epi must be None, 'gelu' or 'residual', got %r" % (epi,))
    if Kw != K or ldw != K or Po != P or No != N or (bias is not None and bias.numel() != N) or \
            (gamma is not None and gamma.numel() != N):
        raise NativeError("vc_linear: shape mismatch X=%s W=%s out=%s" % (tuple(X.shape), tuple(W.shape), tuple(out.shape)))
    r, m = _res("vc_linear", res, out), _hg_map(rowb0)
    _check(load().t2amd_vc_linear_f32(*x, pw, _floats(W), _vec(bias), N, VC_EPI[epi], _vec(gamma), *r, *o, *m,
                                      int(precision), _stream()), "t2amd_vc_linear_f32")


def vc_polar(Y, F, clamp, rowb0, S):
    """S [P][lds] interleaved (re, im) = min(exp(Y[:, k]), clamp) (cos, sin)(Y[:, F + k]) for k < F, zero pad columns and
    halo rows."""
    y, P, Ny = _image(Y)
    s, Ps, Ns = _image(S, True)
    if Ps != P or Ny < 2 * F or Ns != s[1] or Ns < 2 * F:
        raise NativeError("vc_polar: shape mismatch Y=%s S=%s F=%d" % (tuple(Y.shape), tuple(S.shape), F))
    _check(load().t2amd_vc_polar_f32(*y[:4], int(F), _F(clamp), *_hg_map(rowb0), *s, _stream()), "t2amd_vc_polar_f32")


def vc_ola(frames, wsq, utt, hop, trim, out):
    """out (B, 1, T) = the overlap-add of the frame rows [P][L] of every utterance (utt int32 [B][2]: first row, frames),
    trimmed by `trim` samples, over the overlap-added squared window wsq [L]; zero beyond each utterance."""
    f, _, L = _image(frames)
    if out.dim() != 3 or out.shape[1] != 1 or utt.dtype != torch.int32 or tuple(utt.shape) != (out.shape[0], 2) or \
            not utt.is_contiguous() or wsq.numel() != L:
        raise NativeError("vc_ola: shape mismatch frames=%s wsq=%s utt=%s out=%s" % (tuple(frames.shape), tuple(wsq.shape),
                                                                                      tuple(utt.shape), tuple(out.shape)))
    _check(load().t2amd_vc_ola_f32(*f[:4], _vec(wsq), ptr(utt, torch.int32), int(out.shape[0]), int(L), int(hop),
                                   int(trim), ptr(_fullc(out)), out.shape[2], out.numel(), _stream()), "t2amd_vc_ola_f32")


# ---- the backward pass's row kernels (csrc/vocos_bwd.hip) -----------------------------------------------------------------
def vc_bwd_slot_rows():
    """Consecutive rows per partial slot of the vc_*_bwd column sums."""
    return int(load().t2amd_vc_bwd_slot_rows())


def vc_bwd_slots(P):
    """Partial slots of a [P][.] image: what ``wg_partial_sum`` adds in order."""
    return -(-int(P) // vc_bwd_slot_rows())


def _vc_partial(who, partial, floats):
    """The partial-slot buffer's (pointer, floats); a null buffer is left to the entry to refuse."""
    if partial is None:
        return None, 0
    if partial.dim() != 1 or not partial.is_contiguous() or partial.numel() < floats:
        raise NativeError("%s: partial is shorter than its slots: %d floats, %d needed" % (who, partial.numel(), floats))
    return ptr(partial), partial.numel()


def vc_ola_bwd(d_audio, wsq, utt, rowb0, rowr0, hop, trim, d_frames):
    """d_frames [P][L] = the gradient of ``vc_ola``'s frame rows from d_audio (B, 1, T)."""
    f, P, L = _image(d_frames, True)
    if d_audio.dim() != 3 or d_audio.shape[1] != 1 or utt.dtype != torch.int32 or tuple(utt.shape) != (d_audio.shape[0], 2) or \
            not utt.is_contiguous() or wsq.numel() != L:
        raise NativeError("vc_ola_bwd: shape mismatch d_audio=%s wsq=%s utt=%s d_frames=%s"
                          % (tuple(d_audio.shape), tuple(wsq.shape), tuple(utt.shape), tuple(d_frames.shape)))
    m = _hg_map(rowb0, rowr0)
    _check(load().t2amd_vc_ola_bwd_f32(ptr(_fullc(d_audio)), d_audio.shape[2], d_audio.numel(), _vec(wsq), ptr(utt, torch.int32),
                                       int(d_audio.shape[0]), *m, P, int(L), int(hop), int(trim), *f, _stream()),
           "t2amd_vc_ola_bwd_f32")


def vc_polar_bwd(Y, F, clamp, dS, rowb0, dY):
    """dY [P][N] = [d_m | d_p | 0] from the kept head rows Y [P][>= 2F] and dS [P][>= 2F] interleaved (d_re, d_im)."""
    y, P, Ny = _image(Y)
    s, Ps, Ns = _image(dS)
    o, Po, No = _image(dY, True)
    if Ps != P or Po != P or Ny < 2 * F or Ns < 2 * F or No < 2 * F:
        raise NativeError("vc_polar_bwd: shape mismatch Y=%s dS=%s dY=%s F=%d" % (tuple(Y.shape), tuple(dS.shape),
                                                                                   tuple(dY.shape), F))
    _check(load().t2amd_vc_polar_bwd_f32(*y[:4], int(F), _F(clamp), s[0], s[1], s[2], *_hg_map(rowb0), *o, int(No), _stream()),
           "t2amd_vc_polar_bwd_f32")


def vc_gelu_bwd(U, rowb0, dH):
    """dH [P][I] *= GELU'(U [P][I]), in place; zero on halo rows."""
    u, P, I = _image(U)
    o, Po, Io = _image(dH, True)
    if (Po, Io) != (P, I):
        raise NativeError("vc_gelu_bwd: shape mismatch U=%s dH=%s" % (tuple(U.shape), tuple(dH.shape)))
    _check(load().t2amd_vc_gelu_bwd_f32(*u, *_hg_map(rowb0), *o, _stream()), "t2amd_vc_gelu_bwd_f32")


def vc_gamma_bwd(dX, gamma, rowb0, Y2, partial):
    """partial [slots][D] = the column partials of sum_r dX Y2; then Y2 = gamma dX in place."""
    x, P, D = _image(dX)
    o, Po, Do = _image(Y2, True)
    if (Po, Do) != (P, D) or gamma.numel() != D:
        raise NativeError("vc_gamma_bwd: shape mismatch dX=%s gamma=%s Y2=%s" % (tuple(dX.shape), tuple(gamma.shape),
                                                                                  tuple(Y2.shape)))
    _check(load().t2amd_vc_gamma_bwd_f32(*x, _vec(gamma), *_hg_map(rowb0), *o, *_vc_partial("vc_gamma_bwd", partial, vc_bwd_slots(P) * D),
                                         _stream()), "t2amd_vc_gamma_bwd_f32")


def vc_ln_bwd(X, w, conv_bias, ln_w, eps, rowb0, G, dZ, partial):
    """dZ [P][D] = the gradient of ``vc_dwln``'s LayerNorm input from G = d_out (dZ may be G); partial [slots][2 D] = the
    column partials of the norm's weight | bias gradients."""
    x, P, D = _image(X)
    g, Pg, Dg = _image(G)
    o, Po, Do = _image(dZ, True)
    taps = 0 if w is None else int(w.shape[0])
    if (Pg, Dg) != (P, D) or (Po, Do) != (P, D) or ln_w.numel() != D or \
            (w is not None and (w.dim() != 2 or w.shape[1] != D or conv_bias is None or conv_bias.numel() != D)):
        raise NativeError("vc_ln_bwd: shape mismatch X=%s w=%s G=%s dZ=%s" % (tuple(X.shape), None if w is None else
                                                                               tuple(w.shape), tuple(G.shape), tuple(dZ.shape)))
    _check(load().t2amd_vc_ln_bwd_f32(*x, _vec(w), 0 if w is None else w.numel(), _vec(conv_bias) if w is not None else None,
                                      taps, _vec(ln_w), _F(eps), *_hg_map(rowb0), g[0], g[2], g[1], *o,
                                      *_vc_partial("vc_ln_bwd", partial, vc_bwd_slots(P) * 2 * D), _stream()), "t2amd_vc_ln_bwd_f32")


def vc_dw_bwd(dZ, X, w, rowb0, res, dX, partial):
    """dX [P][D] = res + the transposed depthwise product of dZ with w [taps][D] (res None or dX); partial
    [slots][taps + 1][D] = the column partials of the tap | bias gradients."""
    z, P, D = _image(dZ)
    x, Px, Dx = _image(X)
    o, Po, Do = _image(dX, True)
    if (Px, Dx) != (P, D) or (Po, Do) != (P, D) or w.dim() != 2 or w.shape[1] != D:
        raise NativeError("vc_dw_bwd: shape mismatch dZ=%s X=%s w=%s dX=%s" % (tuple(dZ.shape), tuple(X.shape), tuple(w.shape),
                                                                                tuple(dX.shape)))
    r = _res("vc_dw_bwd", res, dX)
    _check(load().t2amd_vc_dw_bwd_f32(*z, x[0], x[1], x[2], _vec(w), w.numel(), int(w.shape[0]), *_hg_map(rowb0), *r, *o,
                                      *_vc_partial("vc_dw_bwd", partial, vc_bwd_slots(P) * (int(w.shape[0]) + 1) * D), _stream()), "t2amd_vc_dw_bwd_f32")


# ----------------------------------------------------------------------------
# optimiser step (csrc/optim.hip)
# ----------------------------------------------------------------------------
def _raw(t):
    v = ptr(t)
    return None if v is None else v.value


def tensor_list(grads, params=None, exp_avgs=None, exp_avg_sqs=None):
    """-> (TensorList, total_blocks).  Every tensor must be contiguous f32 (views at any offset are fine)."""
    n = len(grads)
    if not 0 < n <= MAX_TENSORS:
        raise NativeError("tensor_list: 1..%d tensors per call, got %d" % (MAX_TENSORS, n))
    chunk = int(load().t2amd_optim_chunk())
    L = TensorList()
    blocks = 0
    for i in range(n):
        g = _fullc(grads[i])
        L.grad[i] = _raw(g)
        L.numel[i] = g.numel()
        L.first_block[i] = blocks
        blocks += (g.numel() + chunk - 1) // chunk
        for field, seq in (("param", params), ("exp_avg", exp_avgs), ("exp_avg_sq", exp_avg_sqs)):
            if seq is not None:
                t = _fullc(seq[i])
                if t.numel() != g.numel():
                    raise NativeError("tensor_list: %s[%d] has %d elements, gradient %d" % (field, i, t.numel(), g.numel()))
                getattr(L, field)[i] = _raw(t)
    L.count = n
    return L, blocks


def grad_norm(L, blocks, max_norm, ws, out):
    """out[0] = global L2 norm of the gradients of L, out[1] = clip coefficient.  ws: float64, >= blocks."""
    if ws.dtype != torch.float64 or ws.numel() < blocks or out.numel() < 2:
        raise NativeError("grad_norm: workspace too small")
    _check(load().t2amd_grad_norm_f32(C.byref(L), C.c_float(max_norm), ptr(ws, torch.float64), ptr(out), _stream()),
           "t2amd_grad_norm_f32")


def adam_step(L, hyper, norm_and_coef=None):
    _check(load().t2amd_adam_step_f32(C.byref(L), C.byref(hyper), ptr(norm_and_coef) if norm_and_coef is not None else None,
                                      _stream()), "t2amd_adam_step_f32")
