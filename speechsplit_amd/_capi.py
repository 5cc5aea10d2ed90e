"""ctypes binding of include/speechsplit_amd.h (the C ABI of libspeechsplit_hip.so).

The product path has no CPU fallback: if the HIP library is missing or fails to load, ``lib()`` raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SS_DIAG_LIB=1 (tools/ only): the -DSS_DIAG build with the wrong-result timing experiments compiled in
LIB_PATH = os.environ.get('SS_LIB_PATH') or os.path.join(_HERE, 'lib', 'libspeechsplit_hip_diag.so' if os.environ.get('SS_DIAG_LIB') == '1' else 'libspeechsplit_hip.so')

HP_FIELDS = ('freq', 'dim_neck', 'freq_2', 'dim_neck_2', 'freq_3', 'dim_neck_3', 'dim_enc', 'dim_enc_2', 'dim_enc_3',
             'dim_freq', 'dim_spk_emb', 'dim_f0', 'chs_grp', 'min_len_seg', 'max_len_seg', 'max_len_seq', 'max_len_pad')


class SSHparams(C.Structure):
    _fields_ = [(n, C.c_int) for n in HP_FIELDS]


def hparams_struct(hp):
    """Build the C struct from any attribute bag with the reference's hparams names (hparams.py:9-32)."""
    return SSHparams(**{n: int(getattr(hp, n)) for n in HP_FIELDS})


# flags of ss_*_train_step, the data-parallel steps and ss_*_decode_backward (the header's SS_STEP_*)
SS_STEP_NO_ADAM = 1
SS_STEP_SPLIT_BACKWARD = 2
SS_STEP_SPLIT_NO_JOIN = 4
SS_STEP_ACCUMULATE = 8
SS_STEP_BUCKET = 16

GEMM_DESC_PTRS =('a', 'b', 'c', 'bias', 'amax_a', 'amax_b', 'a_pre', 'b_pre', 'a_pre_scale', 'b_pre_scale', 'part')
GEMM_IMG_DESC_PTRS = ('a', 'b', 'c', 'bias', 'scale_a', 'scale_b', 'part', 'zeros')
GEMM_DESC_LONGS = ('lda', 'a_bstride', 'a_segstride', 'ldb', 'b_bstride', 'b_segstride', 'ldc', 'cstride')
GEMM_DESC_INTS = ('a_seglen', 'b_seglen', 'M', 'N', 'K', 'batch', 'flags', 'want', 'row_period', 'row_off', 'row_lo', 'row_hi', 'ksplit')
GEMM_IMG_DESC_INTS = ('a_seglen', 'b_seglen', 'M', 'N', 'K', 'batch', 'flags', 'row_period', 'row_off', 'row_lo', 'row_hi', 'rm_T', 'rm_TP', 'ksplit', 'cfg',
                      'bf16')


class SSGemmDesc(C.Structure):
    """ss_gemm_desc (test hook ss_op_gemm_desc): every GemmDesc field a product launch sets."""
    _fields_ = [(n, C.c_void_p) for n in GEMM_DESC_PTRS] + [(n, C.c_long) for n in GEMM_DESC_LONGS] + [(n, C.c_int) for n in GEMM_DESC_INTS]


class SSGemmImgDesc(C.Structure):
    """ss_gemm_img_desc (test hook ss_op_gemm_img_desc): the same for ImgGemmDesc."""
    _fields_ = [(n, C.c_void_p) for n in GEMM_IMG_DESC_PTRS] + [(n, C.c_long) for n in GEMM_DESC_LONGS] + [(n, C.c_int) for n in GEMM_IMG_DESC_INTS]


class SSCodeSrc(C.Structure):
    """ss_code_src (test hooks ss_op_dec_in*): one encoder BLSTM output slab feeding the decoder input."""
    _fields_ = [('o', C.c_void_p), ('d_o', C.c_void_p), ('H', C.c_int), ('freq', C.c_int), ('col', C.c_int), ('ld', C.c_int)]


class SSConvPackTask(C.Structure):
    """ss_conv_pack_task (test hook ss_op_conv_pack_many): one conv weight and its packs / images."""
    _fields_ = [(n, C.c_void_p) for n in ('w', 'wf', 'wb', 'wf_img', 'wb_img')] + [(n, C.c_int) for n in ('Co', 'Ci', 'Cp')]


class SSConvUnpackTask(C.Structure):
    """ss_conv_unpack_task (test hook ss_op_conv_unpack_many): one packed weight gradient and the gradient it unpacks into."""
    _fields_ = [('gp', C.c_void_p), ('g', C.c_void_p)] + [(n, C.c_int) for n in ('Co', 'Ci', 'Cp')]


class SSWgradTask(C.Structure):
    """ss_wgrad_task (test hook ss_op_lstm_wgrad_table): one BLSTM layer's operands and gradient outputs."""
    _fields_ = [('dg', C.c_void_p), ('x', C.c_void_p), ('x_ld', C.c_long), ('hout', C.c_void_p), ('h_ld', C.c_long), ('gwih', C.c_void_p),
                ('gwhh', C.c_void_p), ('gb', C.c_void_p), ('H', C.c_int), ('In', C.c_int), ('R', C.c_long)]


class SSOptimExtOp(C.Structure):
    """ss_optim_ext_op (test hook ss_op_optim_ext): the weight-decay / EMA optimiser kernels on the caller's buffers."""
    _fields_ = ([(n, C.c_void_p) for n in ('p', 'm', 'v', 'ema', 'g', 'state', 'skip_status')] + [('lo', C.c_long), ('hi', C.c_long)] +
                [(n, C.c_double) for n in ('lr', 'beta1', 'beta2', 'eps')] + [('step', C.c_long)] +
                [(n, C.c_float) for n in ('grad_scale', 'clip_coef', 'weight_decay')] + [('ema_decay', C.c_double), ('ema_warmup', C.c_int),
                                                                                       ('ema_updates', C.c_long), ('n_runs', C.c_int)] +
                [('run_start', C.POINTER(C.c_long)), ('run_len', C.POINTER(C.c_int)), ('run_decayed', C.POINTER(C.c_int)), ('mode', C.c_int)])


class SSPrepTask(C.Structure):
    """ss_prep_task (test hook ss_op_prep): dst = a + b (b NULL: a copy) over n floats, img (nullable) the image of dst."""
    _fields_ = [('a', C.c_void_p), ('b', C.c_void_p), ('dst', C.c_void_p), ('n', C.c_long), ('img', C.c_void_p)]


# every symbol include/speechsplit_amd.h declares: name -> (restype, argtypes)
_vp, _fp, _ip, _i, _l, _f, _d = C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
SYMBOLS = {
    'ss_last_error': (C.c_char_p, []),
    'ss_abi_version': (_i, []),
    'ss_create': (_vp, [_i, C.POINTER(SSHparams), _i, _i]),
    'ss_destroy': (None, [_vp]),
    'ss_num_params': (_i, [_vp]),
    'ss_param_info': (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_l), C.POINTER(_i), C.POINTER(_l * 3)]),
    'ss_arena_numel': (_l, [_vp]),
    'ss_workspace_bytes': (_l, [_vp]),
    'ss_plan_bytes': (_l, [_vp, _i, _i]),
    'ss_set_workspace': (_i, [_vp, _vp, _l, _vp]),
    'ss_bind': (_i, [_vp, _fp, _fp, _fp, _fp, _vp, _l, _vp]),
    'ss_g3_forward': (_i, [_vp, _fp, _fp, _fp, _fp, _ip, _i, _i, _i, _fp, _vp]),
    'ss_g3_backward': (_i, [_vp, _fp, _vp]),
    'ss_g3_backward_inputs': (_i, [_vp, _fp, _fp, _fp, _fp, _vp]),
    'ss_g3_rhythm': (_i, [_vp, _fp, _i, _i, _fp, _vp]),
    'ss_g3_forward_ragged': (_i, [_vp, _fp, _fp, _fp, _ip, _i, _i, _i, _fp, _vp]),
    'ss_g3_rhythm_ragged': (_i, [_vp, _fp, _ip, _i, _i, _fp, _vp]),
    'ss_g6_forward_ragged': (_i, [_vp, _fp, _fp, _ip, _i, _i, _i, _fp, _vp]),
    'ss_g6_forward': (_i, [_vp, _fp, _fp, _fp, _ip, _i, _i, _i, _fp, _vp]),
    # e, x_f0, x_org, len, B, T, codes_x, codes_r, codes_f0, stream / e, codes_x, codes_r, codes_f0, c_trg, len, B, T, out, stream
    'ss_g3_encode': (_i, [_vp, _fp, _fp, _ip, _i, _i, _fp, _fp, _fp, _vp]),
    'ss_g3_decode': (_i, [_vp, _fp, _fp, _fp, _fp, _ip, _i, _i, _fp, _vp]),
    # e, x_org, f0_trg, len, B, T, codes_r, codes_f0, stream / e, codes_r, codes_f0, len, B, T, out, stream
    'ss_g6_encode': (_i, [_vp, _fp, _fp, _ip, _i, _i, _fp, _fp, _vp]),
    'ss_g6_decode': (_i, [_vp, _fp, _fp, _ip, _i, _i, _fp, _vp]),
    # e, codes_x, codes_r, codes_f0, c_trg, B, T, out, stream / e, d_out, d_codes_x, d_codes_r, d_codes_f0, dc_trg, flags, stream
    'ss_g3_decode_train': (_i, [_vp, _fp, _fp, _fp, _fp, _i, _i, _fp, _vp]),
    'ss_g3_decode_backward': (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _vp]),
    # e, codes_r, codes_f0, B, T, out, stream / e, d_out, d_codes_r, d_codes_f0, flags, stream
    'ss_g6_decode_train': (_i, [_vp, _fp, _fp, _i, _i, _fp, _vp]),
    'ss_g6_decode_backward': (_i, [_vp, _fp, _fp, _fp, _i, _vp]),
    'ss_adam_step_decoder': (_i, [_vp, _f, _vp]),
    # e, codes_x, codes_r, codes_f0, c_trg, target_mel, B, T, grad_scale, flags, loss, dc_trg, stream
    'ss_g3_decode_train_step': (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp, _vp]),
    'ss_g6_backward': (_i, [_vp, _fp, _vp]),
    'ss_g6_backward_inputs': (_i, [_vp, _fp, _fp, _fp, _vp]),
    'ss_g3_train_step': (_i, [_vp, _fp, _fp, _fp, _ip, _fp, _ip, _i, _i, _f, _i, _fp, _vp]),
    'ss_g6_train_step': (_i, [_vp, _fp, _fp, _ip, _fp, _ip, _i, _i, _f, _i, _fp, _vp]),
    'ss_train_finish': (_i, [_vp, _f, _i, _vp]),
    'ss_wait_decoder_grads': (_i, [_vp, _vp]),
    'ss_side_stream': (_vp, [_vp]),
    'ss_grad_split': (_l, [_vp]),
    'ss_stream_report': (C.c_char_p, [_vp]),
    'ss_comm_unique_id': (_i, [C.c_char_p]),
    'ss_comm_init': (_i, [_vp, C.c_char_p, _i, _i]),
    'ss_comm_destroy': (_i, [_vp]),
    'ss_allreduce_grads': (_i, [_vp, _l, _l, _vp]),
    'ss_g3_dp_train_step': (_i, [_vp, _fp, _fp, _fp, _ip, _fp, _ip, _i, _i, _i, _fp, _vp]),
    'ss_g6_dp_train_step': (_i, [_vp, _fp, _fp, _ip, _fp, _ip, _i, _i, _i, _fp, _vp]),
    'ss_set_adam': (_i, [_vp, _d, _d, _d, _d, _l, _vp]),
    'ss_adam_step': (_i, [_vp, _f, _vp]),
    'ss_zero_grads': (_i, [_vp, _vp]),
    'ss_grad_accum_count': (_l, [_vp]),
    'ss_set_grad_clip': (_i, [_vp, _f, _vp]),
    'ss_grad_norm': (_i, [_vp, _f, _fp, _vp]),
    'ss_grad_clip_stats': (_i, [_vp, _fp, _vp]),
    'ss_set_weight_decay': (_i, [_vp, _f, _i, _vp]),
    'ss_set_ema': (_i, [_vp, _fp, _d, _i, _l, _vp]),
    'ss_ema_swap': (_i, [_vp, _vp]),
    'ss_ema_stats': (_i, [_vp, _fp, _vp]),
    'ss_set_lr_schedule': (_i, [_vp, _i, _i, _d, _i, _d, _i, _d, _vp]),
    'ss_lr_stats': (_i, [_vp, _fp, _vp]),
    'ss_interp_forward': (_i, [_vp, _fp, _ip, _fp, _ip, _i, _i, _i, _fp, _ip, _fp, _ip, _vp]),
    'ss_interp_backward': (_i, [_vp, _fp, _i, _i, _i, _fp, _vp]),
    'ss_check': (_i, [_vp, _vp]),
    'ss_status': (C.c_uint, [_vp]),
    'ss_clear_abort': (_i, [_vp, _vp]),
    'ss_set_lockstep': (_i, [_vp, _i]),
    'ss_op_gemm': (_i, [_fp, _l, _fp, _l, _fp, _l, _fp, _i, _i, _i, _i, _i, _vp]),
    'ss_op_lstm_fwd': (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _l, _i, _i, _i, _vp]),
    'ss_op_lstm_fwd_ragged': (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _l, _ip, _i, _i, _i, _vp]),
    'ss_op_lstm_bwd': (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _l, _i, _i, _i, _vp]),
    # gates, whh_f, whh_b, out, csave, scratch, floats, xc, xf, out_img, img_bf16, hi_only, len, B, T, H, stream
    'ss_op_lstm_seq_fwd': (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _l, _fp, _i, _fp, _i, _i, _ip, _i, _i, _i, _vp]),
    # gates, whh_f, whh_b, d_out, csave, scratch, floats, amax, gbias_f, gbias_b, dgs, xf, dimg, img_only, hi_only, B, T, H, stream
    'ss_op_lstm_seq_bwd': (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _l, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _i, _vp]),
    'ss_op_lstm_wgrad': (_i, [_fp, _fp, _l, _fp, _fp, _fp, _fp, _fp, _l, _l, _i, _i, _vp]),
    'ss_op_gn_relu_scratch': (_l, [_i, _i, _i]),
    # x, x_ld, x_bs, y, y_ld, y_bs, gamma, beta, stats, len, i0, lam, nrows, P, y_img, img_scale, img_bf16, scratch, bytes, B, T, C, stream
    'ss_op_gn_relu_fwd': (_i, [_fp, _l, _l, _fp, _l, _l, _fp, _fp, _fp, _ip, _ip, _fp, _ip, _i, _fp, _fp, _i, _vp, _l, _i, _i, _i, _vp]),
    # x, x_ld, x_bs, gamma, beta, stats, mask, B, T, C, stream
    'ss_op_gn_relu_mask': (_i, [_fp, _l, _l, _fp, _fp, _fp, _fp, _i, _i, _i, _vp]),
    # x, x_ld, x_bs, dy, dy_ld, dy_bs, gamma, beta, stats, g_gamma, g_beta, g_bias, amax, part, lam, start, P, src, src_ld, src_bs, dy_img, B, T, C, stream
    'ss_op_gn_relu_bwd': (_i, [_fp, _l, _l, _fp, _l, _l, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _ip, _i, _fp, _l, _l, _fp, _i, _i, _i, _vp]),
    # out, ld, bs, tgt, ld, bs, d_out, ld, bs, B, T, C, grad_scale, partials, loss, stream
    'ss_op_mse_loss': (_i, [_fp, _l, _l, _fp, _l, _l, _fp, _l, _l, _i, _i, _i, _f, _fp, _fp, _vp]),
    # logits, ld, bs, tgt, d_out, ld, bs, B, T, C, grad_scale, partials, loss, stream
    'ss_op_ce_loss': (_i, [_fp, _l, _l, _ip, _fp, _l, _l, _i, _i, _i, _f, _fp, _fp, _vp]),
    'ss_op_colsum_scratch_doubles': (_l, [_i]),
    # in, ld, R, C, two_dir, o0, o1, o2, o3, part, part_doubles, ctr, ctr_words, stream
    'ss_op_colsum': (_i, [_fp, _l, _i, _i, _i, _fp, _fp, _fp, _fp, _vp, _l, _vp, _i, _vp]),
    # src, nsrc, emb, emb_dim, emb_col, dst, ld, B, T, f, stream / src, nsrc, d_in, ld, B, T, f, stream
    'ss_op_dec_in': (_i, [C.POINTER(SSCodeSrc), _i, _fp, _i, _i, _fp, _i, _i, _i, _i, _vp]),
    'ss_op_dec_in_grad': (_i, [C.POINTER(SSCodeSrc), _i, _fp, _i, _i, _i, _i, _vp]),
    'ss_op_dec_in_codes_grad': (_i, [C.POINTER(SSCodeSrc), _i, _fp, _i, _i, _i, _i, _vp]),
    # src, nsrc, emb, emb_dim, emb_col, codes, codes_floats, dst, ld, B, T, f, stream
    'ss_op_dec_in_codes': (_i, [C.POINTER(SSCodeSrc), _i, _fp, _i, _i, _fp, _l, _fp, _i, _i, _i, _i, _vp]),
    # dg, ld, b_stride, rows, w_f, w_r, w_ld, col0, H4, E, out, B, stream
    'ss_op_spk_grad': (_i, [_fp, _l, _l, _i, _fp, _fp, _l, _i, _i, _i, _fp, _i, _vp]),
    # tasks, n, row_groups / tasks, n / tasks, n, row_groups, part, part_floats, ctr, ctr_words, stream
    'ss_op_lstm_wgrad_table_floats': (_l, [C.POINTER(SSWgradTask), _i, _i]),
    'ss_op_lstm_wgrad_table_counters': (_i, [C.POINTER(SSWgradTask), _i]),
    'ss_op_lstm_wgrad_table': (_i, [C.POINTER(SSWgradTask), _i, _i, _fp, _l, _vp, _i, _vp]),
    # scales, len_seg, len_seq, len_seq_const, S, ncand, P, T, B, i0, lam, nrows, counts, start, stream
    'ss_op_interp_plan': (_i, [_fp, _ip, _ip, _i, _i, _i, _i, _i, _i, _ip, _fp, _ip, _ip, _ip, _vp]),
    # i0, lam, nrows, P, x, x_ld, x_bs, y, y_ld, y_bs, C, B, y_img, img_scale, stream
    'ss_op_interp_gather': (_i, [_ip, _fp, _ip, _i, _fp, _l, _l, _fp, _l, _l, _i, _i, _fp, _fp, _vp]),
    # i0, lam, nrows, P, T, mel, f0, CM, ymel, ym_ld, ym_bs, yoh, yo_ld, yo_bs, NOH, qidx, B, stream
    'ss_op_interp_quant': (_i, [_ip, _fp, _ip, _i, _i, _fp, _fp, _i, _fp, _l, _l, _fp, _l, _l, _i, _ip, _i, _vp]),
    # lam, start, P, T, dy, dy_ld, dy_bs, dx, dx_ld, dx_bs, C, B, stream
    'ss_op_interp_scatter': (_i, [_fp, _ip, _i, _i, _fp, _l, _l, _fp, _l, _l, _i, _i, _vp]),
    # w, Co, Ci, Cp, wf, wb, wf_img, wb_img, img_bf16, stream / tasks, n, img_bf16, stream / w, Co, Ci, wb, stream
    'ss_op_conv_pack': (_i, [_fp, _i, _i, _i, _fp, _fp, _fp, _fp, _i, _vp]),
    'ss_op_conv_pack_many': (_i, [C.POINTER(SSConvPackTask), _i, _i, _vp]),
    'ss_op_conv_pack_dx': (_i, [_fp, _i, _i, _fp, _vp]),
    # gp, Co, Ci, Cp, g, acc, stream / tasks, n, acc, stream
    'ss_op_conv_unpack': (_i, [_fp, _i, _i, _i, _fp, _i, _vp]),
    'ss_op_conv_unpack_many': (_i, [C.POINTER(SSConvUnpackTask), _i, _i, _vp]),
    'ss_op_prep': (_i, [C.POINTER(SSPrepTask), _i, _i, _vp]),
    'ss_op_transpose': (_i, [_fp, _i, _i, _fp, _vp]),
    # src, s_ld, s_bs, dst, d_ld, d_bs, len, B, T, C, stream
    'ss_op_copy_rows': (_i, [_fp, _l, _l, _fp, _l, _l, _ip, _i, _i, _i, _vp]),
    # gamma[], beta[], C[], n, T, out, stream / p, n, limit, sticky, stream
    'ss_op_act_scales': (_i, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_i), _i, _i, _fp, _vp]),
    'ss_op_param_guard': (_i, [_fp, _l, _f, _vp, _vp]),
    'ss_op_optim_ext': (_i, [C.POINTER(SSOptimExtOp), _vp]),
    'ss_op_wd_runs': (_i, [_i, C.POINTER(SSHparams), C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int), _i]),
    'ss_op_lr_schedule': (_i, [_i, _d, _i, _d, _i, _d, _i, _d, _vp, _l, _vp, _vp]),
    'ss_op_split_image': (_i, [_fp, _l, _l, _i, _f, _fp, _l, _vp]),
    'ss_op_gemm_pre': (_i, [_fp, _l, _fp, _fp, _l, _fp, _fp, _l, _fp, _i, _i, _i, _i, _i, _vp]),
    'ss_op_gemm_img': (_i, [_fp, _l, _fp, _l, _fp, _l, _fp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _l, _fp, _vp, _vp]),
    'ss_op_gemm_desc': (_i, [C.POINTER(SSGemmDesc), _vp]),
    'ss_op_gemm_img_desc': (_i, [C.POINTER(SSGemmImgDesc), _vp]),
    'ss_op_conv_block_scratch': (_l, [_i, _i, _i, _i]),
    'ss_op_conv_block': (_i, [_fp] * 13 + [_l, _i, _i, _i, _i, _vp]),
    'ss_op_conv_block_ragged': (_i, [_fp] * 5 + [_ip, _fp, _fp, _l, _i, _i, _i, _i, _vp]),
    'ss_debug_relu_mask': (_i, [_vp, C.c_char_p, _fp, _vp]),
    'ss_melspec_frames': (_i, [_i]),
    'ss_melspec': (_i, [_vp, _i, _vp, _i, _fp, _vp]),
    'ss_f0_normalize': (_i, [_vp, _i, _fp, _vp]),
    'ss_pitch_scratch_bytes': (_l, [_i, _i, _d, _d]),
    'ss_pitch_track': (_i, [_vp, _ip, _i, _i, _d, _d, _d, _vp, _vp, _l, _vp]),
    'ss_op_nccf': (_i, [_vp, _ip, _i, _i, _d, _d, _d, _vp, _vp, _vp]),
    'ss_op_pitch_dp': (_i, [_vp, _vp, _ip, _i, _i, _d, _d, _vp, _vp, _l, _vp]),
    'ss_pitch_stat_scratch_bytes': (_l, [_i, _i, _d, _d]),
    'ss_pitch_track_stat': (_i, [_vp, _ip, _i, _i, _d, _d, _d, _vp, _vp, _l, _vp]),
    'ss_op_pitch_stationarity': (_i, [_vp, _ip, _i, _i, _d, _vp, _vp]),
    'ss_op_pitch_dp_stat': (_i, [_vp, _vp, _vp, _ip, _i, _i, _d, _d, _vp, _vp, _l, _vp]),
    'ss_filtfilt_scratch_bytes': (_l, [_i, _i]),
    'ss_filtfilt': (_i, [_vp, _ip, _i, _i, _vp, _vp, _vp, _d, _vp, _d, _vp, _vp, _l, _vp]),
    'ss_melspec_batch': (_i, [_vp, _ip, _i, _i, _vp, _i, _fp, _vp]),
    'ss_f0_normalize_batch': (_i, [_vp, _ip, _i, _i, _d, _fp, _vp]),
    'ss_resample_len': (_l, [_l, _i, _i]),
    'ss_resample_scratch_bytes': (_l, [_i, _i]),
    'ss_resample': (_i, [_vp, _ip, _i, _i, _i, _i, _vp, _i, _vp, _vp, _l, _vp]),
    # B, max_n / x, n, B, max_n, ratio, hang, edge, pause, g (host), y, m, inv, k, scratch, bytes, stream
    'ss_silence_scratch_bytes': (_l, [_i, _i]),
    'ss_remove_silence': (_i, [_vp, _ip, _i, _i, _d, _i, _i, _i, C.POINTER(_d), _vp, _ip, _ip, _ip, _vp, _l, _vp]),
    # x, n, B, max_n, e, stream / e, j, B, max_j, ratio, hang, edge, pause, inv, k, stream / x, n, B, max_n, inv, k, g (host), y, m, stream
    'ss_op_silence_levels': (_i, [_vp, _ip, _i, _i, _vp, _vp]),
    'ss_op_silence_mask': (_i, [_vp, _ip, _i, _i, _d, _i, _i, _i, _ip, _ip, _vp]),
    'ss_op_silence_gather': (_i, [_vp, _ip, _i, _i, _ip, _ip, C.POINTER(_d), _vp, _ip, _vp]),
    'ss_mt19937_rand': (_i, [_vp, _l, _vp, _vp]),
    'ss_dither_rows': (_i, [_vp, _l, _vp, _ip, _i, _i, _vp, _vp]),
    'ss_griffinlim_samples': (_i, [_i]),
    'ss_griffinlim_scratch_bytes': (_l, [_i, _i]),
    'ss_mel_to_linear': (_i, [_fp, _vp, _ip, _i, _i, _i, _d, _vp, _vp]),
    'ss_griffinlim': (_i, [_vp, _vp, _ip, _i, _i, _i, _d, _vp, _vp, _l, _vp]),
    # basis_host, n_mels, packed_host, cap / mel, inv_basis, packed, packed_doubles, frames, B, max_frames, n_mels, n_iter, step, floor, mag, stream
    'ss_mel_nnls_pack': (_l, [_vp, _i, _vp, _l]),
    'ss_mel_to_linear_nnls': (_i, [_fp, _vp, _vp, _l, _ip, _i, _i, _i, _i, _d, _d, _vp, _vp]),
    # mel, f0_hz, inv_basis, packed, packed_doubles, frames, B, max_frames, n_mels, f_top, n_iter, floor, mag, share, stream
    'ss_mel_to_linear_harmonic': (_i, [_fp, _vp, _vp, _vp, _l, _ip, _i, _i, _i, _d, _i, _d, _vp, _vp, _vp]),
    'ss_harmonic_phase_scratch_bytes': (_l, [_i, _i]),
    # f0_hz, share, rand_phase, frames, B, max_frames, f_top, phase0, scratch, scratch_bytes, stream
    'ss_harmonic_phase': (_i, [_vp, _vp, _vp, _ip, _i, _i, _d, _vp, _vp, _l, _vp]),
    'ss_op_harmonic_u': (_i, [_vp, _ip, _i, _i, _vp, _vp]),
    'ss_op_stft': (_i, [_vp, _ip, _i, _i, _vp, _vp]),
    'ss_op_istft': (_i, [_vp, _ip, _i, _i, _vp, _vp, _l, _vp]),
    # mel, len, B, max_t, n_mels, dct, n_ceps, out, stream / fx, tx, fy, ty, B, max_tx, max_ty, dim, scale, out, path, path_len, scratch, bytes, stream
    'ss_mel_cepstra': (_i, [_fp, _ip, _i, _i, _i, _vp, _i, _vp, _vp]),
    'ss_dtw_scratch_bytes': (_l, [_i, _i, _i]),
    'ss_dtw': (_i, [_vp, _ip, _vp, _ip, _i, _i, _i, _i, _d, _vp, _ip, _ip, _vp, _l, _vp]),
    # path, path_len, f0x, f0y, B, max_tx, max_ty, out, stream
    'ss_path_f0_stats': (_i, [_ip, _ip, _vp, _vp, _i, _i, _i, _vp, _vp]),
    # B, max_n / x, y, n, B, max_n, band_lo (host), band_hi (host), n_bands, extended, out, scratch, bytes, stream
    'ss_stoi_scratch_bytes': (_l, [_i, _i]),
    'ss_stoi': (_i, [_vp, _vp, _ip, _i, _i, C.POINTER(_i), C.POINTER(_i), _i, _i, _vp, _vp, _l, _vp]),
    # x, y, n, B, max_n, from_map, e, inv, k, xp, yp, stream / sig, len, B, max_len, band_lo (host), band_hi (host), n_bands, env, stream
    'ss_op_stoi_compact': (_i, [_vp, _vp, _ip, _i, _i, _i, _vp, _ip, _ip, _vp, _vp, _vp]),
    'ss_op_stoi_bands': (_i, [_vp, _ip, _i, _i, C.POINTER(_i), C.POINTER(_i), _i, _vp, _vp]),
    'ss_collate': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'ss_set_precision': (_i, [_vp, _i]),
    'ss_profile': (_i, [_vp, C.c_uint]),
    'ss_profile_sample': (_i, [_vp, _i]),
    'ss_scratch_fallbacks': (_l, [_vp]),
    'ss_dp_profile': (_i, [_vp, _i]),
    'ss_dp_profile_read': (_i, [_vp, C.POINTER(C.c_double), _i]),
    'ss_profile_read': (_i, [_vp, _i, C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'ss_profile_timeline': (_i, [_vp, C.POINTER(C.c_double), _i]),
    'ss_debug_gemm_phases': (_i, [C.POINTER(C.c_ulonglong), _i]),
    'ss_debug_xcc_map': (_i, [_i, _i, _i, _i, _vp, _vp]),
    'ss_debug_img_wq': (_i, [C.POINTER(C.c_uint), _i]),
    'ss_tune': (_i, [C.c_char_p, _i]),
    'ss_debug_buffer': (_i, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_l), C.POINTER(_l)]),
    'ss_debug_names': (_i, [_vp, C.c_char_p, _i]),
    'ss_debug_last_variant': (_i, [C.c_char_p, C.c_char_p, _i]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'(or `make -C speechsplit_amd/csrc`).  There is no CPU fallback for the engine.')
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(h, name)          # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = h
        # SS_TUNE="key=value,key=value": experiment knobs applied once at load (A/B runs of the tests and tools against a non-default schedule)
        for kv in filter(None, os.environ.get('SS_TUNE', '').split(',')):
            k, v = kv.split('=')
            if h.ss_tune(k.strip().encode(), int(v)) != 0:
                raise RuntimeError('speechsplit_amd: SS_TUNE: ' + h.ss_last_error().decode())
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError('speechsplit_amd: ' + lib().ss_last_error().decode())
