// The process-global knobs (ss_tune keys) that are read outside the file defining them.  Each definition, with the comment that says what
// the values mean and what was measured, stays beside the code it steers.
#pragma once

namespace ss {

extern int g_gemm_want, g_deterministic, g_gemm_diag;                                  // gemm_f32.hip
extern int g_gemm_tr, g_gemm_ws, g_gemm_mode, g_gemm_pipe;                             // gemm_bf16x3.hip
extern int g_small_lds;                                                                // lstm_small.hip
extern int g_lstm_nw, g_lstm_g, g_lstm_mode;                                           // lstm_step.hip
extern int g_seq_prio, g_seq_tag, g_seq_var, g_seq_spin_log2;                          // lstm_seq.hip
// engine.hip (read by ss_tune and the LSTM test hooks, abi_ops.hip)
extern int g_fwd_f16x2, g_bwd_f16x2, g_overlap, g_dx_batched, g_defer_dw, g_dp_emulate, g_dp_model, g_dp_buckets, g_bf16_img, g_compact0;
extern int g_persist, g_own_streams, g_prio_order, g_probe_queues, g_gn_gather, g_conv_dw_off, g_dec_tail_split, g_early_dw, g_xcd_dw;

}  // namespace ss
