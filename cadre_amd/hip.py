"""ctypes binding of libcadre_hip.so (include/cadre_hip.h) + thin tensor-pointer helpers.

PyTorch-ROCm is plumbing here: it owns device memory and streams; every call below hands
raw device pointers and the current HIP stream to the C ABI.  There is NO CPU fallback:
a missing library raises at first use (`lib()`), and every kernel wrapper requires device
tensors.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CADRE_HIP_LIB") or os.path.join(_HERE, "csrc", "libcadre_hip.so")
_lib = None

i32, i64, f32, f64, vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p


class GemmDesc(C.Structure):
    _fields_ = [("A", vp), ("B", vp), ("C", vp), ("scale", vp), ("shift", vp), ("resid", vp),
                ("lda", i64), ("ldb", i64), ("ldc", i64), ("ldr", i64),
                ("M", i32), ("N", i32), ("K", i32), ("a_mode", i32), ("b_mode", i32),
                ("act", i32), ("slope", f32), ("batch", i32),
                ("a_div", i32), ("a_mod", i32), ("b_div", i32), ("b_mod", i32), ("c_div", i32), ("c_mod", i32),
                ("s_div", i32), ("s_mod", i32), ("r_div", i32), ("r_mod", i32),
                ("a_str", i64), ("b_str", i64), ("c_str", i64), ("s_str", i64), ("r_str", i64),
                ("H", i32), ("W", i32), ("Cin", i32), ("Ho", i32), ("Wo", i32), ("KH", i32), ("KW", i32),
                ("stride", i32), ("pad", i32), ("split_k", i32), ("tile", i32), ("flags", i32), ("seg_mode", i32),
                ("row_seg", vp), ("seg_period", i32), ("seg_div", i32)]


# name -> argtypes (restype is int unless noted); must list every symbol of include/cadre_hip.h
SYMBOLS = {
    "cadre_abi_version": [],
    "cadre_last_error": [],
    "cadre_gemm_f32": [C.POINTER(GemmDesc), vp],
    "cadre_gemm_pick_tile": [C.POINTER(GemmDesc)],
    "cadre_gemm_bf16": [C.POINTER(GemmDesc), vp],
    "cadre_gemm_bf16_pick_tile": [C.POINTER(GemmDesc)],
    "cadre_conv3x3_ring": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "cadre_conv3x3_ring_supported": [i32, i32, i32, i32, i32, i32],
    "cadre_conv3x3_ring_ntile": [i32, i32, i32, i32, i32, i32],
    "cadre_conv3x3_s2": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "cadre_conv3x3_s2_supported": [i32, i32, i32, i32, i32],
    "cadre_conv3x3_s1x": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "cadre_conv3x3_s1x_supported": [i32, i32, i32, i32, i32, i32],
    "cadre_conv3x3_s1x_stages": [i32, i32],
    "cadre_gemm_bf16_w128": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "cadre_gemm_bf16_w128_supported": [i32, i32, i32, i32, i32, i32],
    "cadre_maxpool3x3s2_bf16": [vp, vp, i32, i32, i32, i32, vp],
    "cadre_pam_bf16out": [vp, vp, f32, vp, i32, i32, vp],
    "cadre_cam_bf16out": [vp, f32, vp, i32, i32, vp],
    "cadre_splitk_reduce": [vp, i32, i64, i64, vp, i64, i32, i32, vp, vp, i32, f32, vp, i32, vp],
    "cadre_preprocess": [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
    "cadre_preprocess_bf16pad": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "cadre_maxpool3x3s2": [vp, vp, i32, i32, i32, i32, vp],
    "cadre_pack_obs": [vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp],
    "cadre_stem_pool": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, i64, i32, i64, vp],
    "cadre_div255_selfcheck": [vp, vp, vp],
    "cadre_stem_pool_supported": [i32, i32],
    "cadre_winograd_c64": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "cadre_winograd_in": [vp, vp, i32, i32, i32, i32, i32, vp],
    "cadre_winograd_out": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "cadre_winograd_fused_supported": [i32, i32, i32, i32, i32, i32],
    "cadre_winograd_fused_capable": [i32, i32, i32, i32, i32, i32],
    "cadre_winograd_fused_ntb": [i32, i32],
    "cadre_winograd_frag_elems": [i32, i32, i32, i32, i32],
    "cadre_winograd_in_frag": [vp, vp, i32, i32, i32, i32, i32, vp],
    "cadre_winograd_gemm_out": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "cadre_pam": [vp, vp, f32, vp, i32, i32, vp],
    "cadre_cam": [vp, f32, vp, i32, i32, vp],
    "cadre_intertask_att": [vp, vp, i64, i32, f32, vp],
    "cadre_append_measurements": [vp, vp, i64, i32, vp],
    "cadre_gae": [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, i32, vp],
    "cadre_gather_obs": [vp, i64, i32, vp, i32, vp, i64, i32, vp],
    "cadre_gather_minibatch": [vp, i64, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32,
                               vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp],
    "cadre_gather_minibatch_multi": [vp, i32, i64, i32, i64, vp, i32, i32, i32, i32, vp, i64, i64, vp, vp, i64, i64,
                                     vp, vp, vp, vp, vp, vp, vp],
    "cadre_gather_sorted_multi": [vp, i32, i64, i32, i64, vp, i32, i32, i32, i32, i32, vp, i64, i64, vp, vp, i64, i64,
                                  vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "cadre_pack_lstm_weights": [vp, i64, i32, i32, i32, vp, vp, i64, vp],
    "cadre_lstm_step_fwd": [vp, i64, vp, i64, vp, i32, i64, vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, vp, i32, vp],
    "cadre_lstm_step_bwd": [vp, i64, vp, vp, i64, vp, vp, i32, i64, vp, vp, i64, vp, vp, i32, i64, i32, i32, i32, vp, i32, vp, i32, vp],
    "cadre_mlp_fwd": [vp, i64, vp, vp, i32, i64, vp, vp, vp, i32, i32, vp, vp],
    "cadre_mlp_bwd": [vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, i32, vp, vp],
    "cadre_mlp_dw": [vp, vp, vp, vp, vp, vp, i32, i64, vp, i64, vp, i32, i32, vp, vp],
    "cadre_lstm_dw": [vp, i32, i64, vp, vp, i32, i64, i64, i32, vp, vp, vp, vp, i32, i64, i32, i32, i32, i32, i32, vp, vp],
    "cadre_colsum": [vp, i64, i64, vp, i64, i32, i32, i32, i32, vp],
    "cadre_relu_bwd": [vp, vp, i64, vp, i32, i32, i32, vp],
    "cadre_lstm_init": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp],
    "cadre_mfma_peak": [i32, i32, i32, vp, vp],
    "cadre_hbm_stream": [i32, vp, vp, i64, vp, vp],
    "cadre_mfma_shape": [i32, i32, i32, vp, vp],
    "cadre_sort_rows_by_command": [vp, i32, i32, vp, vp, vp],
    "cadre_permute_minibatch": [vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i64, vp],
    "cadre_ppo_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp],
    "cadre_ppo_loss_stats": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp,
                             vp, vp, vp, i32, vp, f32, vp, vp],
    "cadre_grad_norms": [vp, i32, vp, i32, vp],
    "cadre_ppo_loss_hp": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, vp, vp, vp, vp, vp, vp],
    "cadre_ppo_loss_stats_hp": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, vp, vp, vp, vp, vp,
                                vp, i32, vp, f32, vp, vp],
    "cadre_grad_norms_hp": [vp, i32, vp, i32, vp, vp],
    "cadre_explained_variance": [vp, i32, vp, vp],
    "cadre_sample": [vp, i64, vp, i64, i32, i32, vp, vp, vp],
    "cadre_act_windows": [vp, i64, i32, vp, i64, i32, vp, vp, vp, vp, i32, i32, vp, i64, i32, vp, i64, vp],
    "cadre_sample_rows": [vp, i64, i64, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp],
    "cadre_insert_rows": [vp, vp, i32, i32, i64, i64, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp],
    "cadre_categorical_eval": [vp, i64, vp, i32, i32, vp, vp, vp],
    "cadre_categorical_dist": [vp, i64, i32, i32, vp, vp, vp, vp],
    "cadre_clip_adam": [vp, vp, vp, vp, vp, i32, vp, f64, f64, f64, f64, f64, i32, vp],
    "cadre_clip_adam_graph": [vp, vp, vp, vp, vp, i32, vp, f64, f64, f64, f64, f64, vp, vp],
    "cadre_clip_adam_pack_graph": [vp, vp, vp, vp, vp, i32, vp, f64, f64, f64, f64, f64, vp, i32, i64, i64, i32, i32, i32, vp, vp, i64, vp],
    "cadre_clip_adam_graph_gated": [vp, vp, vp, vp, vp, i32, vp, f64, f64, f64, f64, f64, vp, vp, vp],
    "cadre_clip_adam_pack_graph_gated": [vp, vp, vp, vp, vp, i32, vp, f64, f64, f64, f64, f64, vp, i32, i64, i64, i32, i32, i32, vp, vp,
                                         i64, vp, vp],
    "cadre_clip_adam_norms": [vp, vp, i32, vp, f64, f64, f64, vp, i64, i64, vp],
    "cadre_clip_adam_apply": [vp, vp, vp, vp, vp, i32, vp, f64, f64, f64, f64, i64, i64, vp],
    "cadre_clip_adam_graph_hp": [vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, f64, vp, vp],
    "cadre_clip_adam_graph_hp_gated": [vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, f64, vp, vp, vp],
    "cadre_clip_adam_pack_graph_hp": [vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, f64, vp, i32, i64, i64, i32, i32, i32, vp, vp, i64, vp],
    "cadre_clip_adam_pack_graph_hp_gated": [vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, f64, vp, i32, i64, i64, i32, i32, i32, vp, vp,
                                            i64, vp, vp],
    "cadre_clip_adam_norms_hp": [vp, vp, i32, vp, vp, f64, f64, vp, i64, i64, vp],
    "cadre_clip_adam_apply_hp": [vp, vp, vp, vp, vp, i32, vp, vp, f64, f64, f64, i64, i64, vp],
    "cadre_return_stats": [vp, i32, i32, f64, f64, i32, vp, vp, vp],
    "cadre_gae_multi": [vp, i32, i32, f32, f32, i32, vp, f32, vp],
    "cadre_insert_rows_tl": [vp, vp, i32, i32, i64, i64, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp],
    # ordinal policy heads (the rank table `ord` is the argument before the stream)
    "cadre_ppo_loss_ord": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, f32, f32, f32, f32,
                           vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp, vp],
    "cadre_sample_ord": [vp, i64, vp, i64, i32, i32, vp, vp, vp, vp],
    "cadre_sample_rows_ord": [vp, i64, i64, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp],
    "cadre_categorical_eval_ord": [vp, i64, vp, i32, i32, vp, vp, vp, vp],
    "cadre_categorical_dist_ord": [vp, i64, i32, i32, vp, vp, vp, vp, vp],
    # training checkpoints: range table, n_ranges, staging (NULL: digests only), digests, stream
    "cadre_state_capture": [vp, i32, vp, vp, vp],
    # rank consensus: reduced kl pair, target_kl, stop, desired_kl, hp, stats row, F, stream / per-rank statistics, world,
    # epsilon, state, merged (may be NULL), stream
    "cadre_kl_consensus": [vp, f32, vp, f64, vp, vp, i32, vp],
    "cadre_return_scale_merge": [vp, i32, f64, vp, vp, vp],
    # ensemble evaluation: O3, ldo, z_str, pos, cmd, N, C, Mg, m0, M, q (NULL: greedy), K_steer, K_throttle, action, logp,
    # value, ord (may be NULL), stream / action, N, M, steer table, K_steer, throttle table, K_throttle, controls, stream
    "cadre_sample_rows_ens": [vp, i64, i64, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp],
    "cadre_ensemble_controls": [vp, i32, i32, vp, i32, vp, i32, vp, vp],
    # behaviour cloning: logits, ldl, l_ns, values, ldv, v_ns, actions, commands, returns, weights (may be NULL), B, C, K_steer,
    # K_throttle, label_smoothing, bc_coeff, value_coeff, ent_coeff, inv_b, losses, dlogits, dvalues (both NULL: evaluation),
    # scratch, poison, stats row (may be NULL), F, stats scratch, ord (may be NULL), stream / latent, ld_lat, n_frames, window,
    # meas, T, S, obs, ldo, stream
    "cadre_bc_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp,
                      vp, vp, vp, i32, vp, vp, vp],
    "cadre_demo_rows": [vp, i64, i32, vp, vp, i32, i32, vp, i64, vp],
    # demonstration term inside the PPO step: logits, ldl, l_ns, values, ldv, v_ns, actions, commands, old_values, returns,
    # old_logp, adv (PPO rows: advantage, demonstration rows: weight), row_kind, B, C, K_steer, K_throttle, hp (may be NULL),
    # clip, value_coeff, clip_coeff, ent_coeff, inv_b, label_smoothing, demo_coeff, demo_value_coeff, inv_bd, losses[3],
    # demo_losses[2], dlogits, dvalues, scratch, demo scratch, poison, PPO stats row (may be NULL), F, stats scratch, target_kl,
    # stop, demo stats row (may be NULL), demo F, ord (may be NULL), stream / pos (NULL: identity), B, B_ppo, row_kind, stream
    "cadre_ppo_demo_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, f32, f32, f32,
                            f32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp, i32, vp, vp],
    "cadre_mix_row_kinds": [vp, i32, i32, vp, vp],
    # PPG auxiliary phase: logits, ldl, l_ns, commands, pos (NULL: identity), row_id, B, C, K_steer, K_throttle, ord (may be
    # NULL), table, R, stream / logits, ldl, l_ns, values, ldv, v_ns, commands, returns, pos (NULL: identity), row_id, table, R,
    # B, C, K_steer, K_throttle, beta_clone, aux_value_coeff, inv_b, losses, dlogits, dvalues, scratch, poison, stats row (may
    # be NULL), F, stats scratch, ord (may be NULL), stream
    "cadre_aux_record": [vp, i64, i64, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp],
    "cadre_aux_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, f32, vp, vp, vp,
                       vp, vp, vp, i32, vp, vp, vp],
    # sample reuse: logits, ldl, l_ns, values, ldv, v_ns, commands, actions, pos (NULL: identity), row_id, B, C, K_steer,
    # K_throttle, ord (may be NULL), logp_now, value_now, R, stream / row table, n, T, gamma, gamma_tau, normalise, state (may be
    # NULL), clip_r, rho_bar, c_bar, stream
    "cadre_reuse_record": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp],
    "cadre_vtrace_multi": [vp, i32, i32, f32, f32, i32, vp, f32, f32, f32, vp],
    # exploration suggestions: events pointer table, slots, codes, n, T, stream / {events, masks, time_limits or 0, suggest}
    # table, n, T, Z, horizon, stream / suggest pointer table, n_src, idx, Bw, T, pos (NULL: identity), Bt, kind, stream /
    # logits, ldl, l_ns, values, ldv, v_ns, actions, commands, old_values, returns, old_logp, adv, kind, prior, Z, B, C, K_steer,
    # K_throttle, hp (may be NULL), clip, value_coeff, clip_coeff, ent_coeff, inv_b, sug_coeff, losses[3], sug_losses[1],
    # dlogits, dvalues, scratch, suggestion scratch, poison, PPO stats row (may be NULL), F, stats scratch, target_kl, stop,
    # suggestion stats row (may be NULL), its F, ord, stream
    "cadre_suggest_note": [vp, vp, vp, i32, i32, vp],
    "cadre_suggest_mark": [vp, i32, i32, i32, vp, vp],
    "cadre_suggest_rows": [vp, i32, vp, i32, i32, vp, i32, vp, vp],
    "cadre_ppo_sug_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, f32, f32,
                           f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp, i32, vp, vp],
    # frame-table storages: the four gathers with window ids (obs, win (NULL: materialised), n_frames, then the twin's
    # arguments; the multi forms: records of eleven words, see the header) / obs pointer table, n, P, S, ldo, D, flags,
    # win_local, count, stream / ..., flags, win_local, base, frames, ld, F_cap, win_dst, row0, stream
    "cadre_gather_obs_ft": [vp, vp, i64, i64, i32, vp, i32, vp, i64, i32, vp],
    "cadre_gather_minibatch_ft": [vp, vp, i64, i64, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32,
                                  vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp],
    "cadre_gather_minibatch_multi_ft": [vp, i32, i64, i32, i64, vp, i32, i32, i32, i32, vp, i64, i64, vp, vp, i64, i64,
                                        vp, vp, vp, vp, vp, vp, vp],
    "cadre_gather_sorted_multi_ft": [vp, i32, i64, i32, i64, vp, i32, i32, i32, i32, i32, vp, i64, i64, vp, vp, i64, i64,
                                     vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "cadre_frames_scan": [vp, i32, i32, i32, i64, i32, vp, vp, vp, vp],
    "cadre_frames_copy": [vp, i32, i32, i32, i64, i32, vp, vp, vp, vp, i64, i64, vp, vp, vp],
    "cadre_deconv3x3_s2_supported": [i32, i32, i32, i32, i32, i32, i32, i32],
    "cadre_deconv3x3_s2": [vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp],
    "cadre_deconv3x3_s2_out": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "cadre_argmax_rows": [vp, i64, i32, i32, vp, vp],
    "cadre_bc_head": [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, vp],
    # self-imitation: logits, ldl, l_ns, values, ldv, v_ns, actions, commands, old_values, returns, old_logp, adv, row_kind, B,
    # C, K_steer, K_throttle, hp (may be NULL), clip, value_coeff, clip_coeff, ent_coeff, inv_b, sil_coeff, sil_value_coeff,
    # inv_bs, losses[3], sil_losses[2], sil_w, dlogits, dvalues, scratch, SIL scratch, poison, PPO stats row (may be NULL), F,
    # stats scratch, target_kl, stop, SIL stats row (may be NULL), its F, ord, stream / {rewards, masks, time_limits or 0,
    # value_preds, returns, flags, q} table, n, T, gamma, state (may be NULL), clip_r, tail, alpha, prio_eps, stream /
    # q, Rcap, filled rows, u, n, idx, scratch, stream / q, Rcap, idx, n, sil_w, pos (NULL: identity), B, B_ppo, alpha,
    # prio_eps, stream
    "cadre_ppo_sil_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, f32, f32, f32,
                           f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp, i32, vp, vp],
    "cadre_sil_prepare": [vp, i32, i32, f32, vp, f32, i32, f64, f64, vp],
    "cadre_sil_draw": [vp, i64, i64, vp, i32, vp, vp, vp],
    "cadre_sil_scatter": [vp, i64, vp, i32, vp, vp, i32, i32, f64, f64, vp],
    # temporal smoothness: {masks, time_limits or 0, command} table, idx, nW, E, Bw, T, C, rotation, pos (NULL: identity), Bt,
    # row_kind, mate, stream / logits, ldl, l_ns, values, ldv, v_ns, actions, commands, old_values, returns, old_logp, adv,
    # row_kind, mate, ctrl, B, C, K_steer, K_throttle, hp (may be NULL), clip, value_coeff, clip_coeff, ent_coeff, inv_b,
    # smooth_coeff, scale_steer, scale_throttle, inv_bp, losses[3], smooth_losses[1], smooth_d, dlogits, dvalues, scratch,
    # smoothness scratch, poison, PPO stats row (may be NULL), F, stats scratch, target_kl, stop, smoothness stats row (may be
    # NULL), its F, ord, stream / {action, masks, time_limits or 0, command} table, n, T, C, K_steer, K_throttle, ctrl, out, stream
    "cadre_smooth_mates": [vp, vp, i32, i32, i32, i32, i32, i64, vp, i32, vp, vp, vp],
    "cadre_ppo_smooth_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, f32, f32,
                              f32, f32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp, i32, vp, vp],
    "cadre_action_jitter": [vp, i32, i32, i32, i32, i32, vp, vp, vp],
    # curiosity (random network distillation): obs table, N, T, S, ldo, D, update, state, stream / obs table, N, T, S, ldo, D, H, E,
    # row0, rows, state, eps_obs, clip, target, predictor, err, xh, h1, h2, diff (the last four may be NULL), stream / err, N, T,
    # {rewards, mixed} table, state, D, gamma, eps, update, stream / xh, h1, h2, diff, err, rows, D, H, E, predictor, state, thresh,
    # grads, loss[2], scratch, stream
    "cadre_rnd_obs_stats": [vp, i32, i32, i32, i64, i32, i32, vp, vp],
    "cadre_rnd_forward": [vp, i32, i32, i32, i64, i32, i32, i32, i32, i32, vp, f64, f32, vp, vp, vp, vp, vp, vp, vp, vp],
    "cadre_rnd_reward": [vp, i32, i32, vp, vp, i32, f64, f64, i32, vp],
    "cadre_rnd_backward": [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp],
    # action masks: the `_ord` twins with the words `allowed` before the stream / allowed pointer table, slots, words, n, T,
    # stream / allowed pointer table, n_src, idx, Bw, T, pos (NULL: identity), B, out, stream / the arguments of
    # cadre_ppo_loss_ord, then allowed, mask stats row (may be NULL), its F, mask scratch, stream
    "cadre_sample_am": [vp, i64, vp, i64, i32, i32, vp, vp, vp, vp, vp],
    "cadre_sample_rows_am": [vp, i64, i64, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp],
    "cadre_categorical_eval_am": [vp, i64, vp, i32, i32, vp, vp, vp, vp, vp],
    "cadre_allowed_note": [vp, vp, vp, i32, i32, vp],
    "cadre_allowed_rows": [vp, i32, vp, i32, i32, vp, i32, vp, vp],
    "cadre_ppo_am_loss": [vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, f32, f32, f32, f32,
                          vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp, vp, vp, i32, vp, vp],
    # cost constraints (PPO-Lagrangian): costs pointer table, slots, costs, n, T, stream / obs table (one head), n, Tr, S, ldo, D, H,
    # row0, rows, tower, values, h1, h2 (both may be NULL), stream / obs table, n, Tr, S, ldo, D, H, row0, rows, tower, values, h1, h2,
    # returns, ldr, grads, loss[2], scratch, stream / costs pointer table, N, T, state, update, stream / {cost_adv, advantages}
    # table, n, T, state, diag (may be NULL), stream
    "cadre_cost_note": [vp, vp, vp, i32, i32, vp],
    "cadre_cost_forward": [vp, i32, i32, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp],
    "cadre_cost_backward": [vp, i32, i32, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp],
    "cadre_cost_lambda": [vp, i32, i32, vp, i32, vp],
    "cadre_lag_mix": [vp, i32, i32, vp, vp, vp],
    # weight averaging: params, ema, seg_off, n_models, state, work, stop (may be NULL), stream / a, b, n, stream / source
    # pointer table, weights, K, out, n, stream
    "cadre_ema_update": [vp, vp, vp, i32, vp, vp, vp, vp],
    "cadre_arena_swap": [vp, vp, i64, vp],
    "cadre_arena_mean": [vp, vp, i32, vp, i64, vp],
}
# entry points of the A/B build only (include/cadre_hip_ab.h; CADRE_BUILD_AB=1 python -m cadre_amd.build, then
# CADRE_HIP_LIB=.../libcadre_hip_ab.so): bound when the loaded library has them
AB_SYMBOLS = {
    "cadre_lstm_pointwise_fwd": [vp, i64, i64, vp, i64, i32, vp, vp, vp, i64, i64, i32, i32, i32, vp, vp],
    "cadre_lstm_pointwise_bwd": [vp, vp, i64, i64, vp, vp, i64, vp, vp, i64, i32, i64, i64, i32, i32, i32, vp, i32, vp, vp],
    "cadre_colsum2": [vp, i64, i64, vp, vp, i64, i32, i32, i32, vp, i32, vp],
    "cadre_conv3x3_c64_bf16": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "cadre_lstm_seq_fwd": [vp, i64, vp, i64, vp, i32, i64, vp, vp, vp, i32, i64, i32, i32, i32, i32, vp, vp, vp],
    "cadre_conv3x3_w128": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "cadre_conv3x3_w128_supported": [i32, i32, i32, i32, i32],
}


ABI_VERSION = 15


class CadreHipError(RuntimeError):
    pass


def has_ab_kernels():
    """True when the loaded library is the A/B build (superseded kernels of csrc/ab/ present)."""
    return hasattr(lib(), "cadre_conv3x3_c64_bf16")


def lib():
    """Load the HIP library; fail loudly if it is missing (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CadreHipError(
                "libcadre_hip.so not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python -m cadre_amd.build`. There is no CPU fallback for the Cadre MI355X learner." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, args in SYMBOLS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_char_p if name == "cadre_last_error" else (C.c_int64 if name == "cadre_winograd_frag_elems" else C.c_int)
        if L.cadre_abi_version() != ABI_VERSION:
            raise CadreHipError("libcadre_hip.so ABI version mismatch (library %d, binding %d): rebuild with "
                                "`python -m cadre_amd.build`" % (L.cadre_abi_version(), ABI_VERSION))
        for name, args in AB_SYMBOLS.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.argtypes = args
                fn.restype = C.c_int
        _lib = L
    return _lib


# the hyper-parameter block of the `_hp` entry points (CADRE_HP_* of include/cadre_hip.h): field name -> index
HP_FIELDS = 16
HP = dict(lr=0, clip=1, value_coeff=2, clip_coeff=3, ent_coeff=4, max_grad_norm=5, desired_kl=6, lr_min=7, lr_max=8, lr_factor=9)
# two of the block's reserved fields, read by cadre_ppo_demo_loss only (the enumerators CADRE_HP_DEMO_COEFF /
# CADRE_HP_DEMO_VALUE_COEFF of the header); HP_INDEX: every named field, what PPOLearnerHIP.set_hyper looks names up in
HP_DEMO_COEFF, HP_DEMO_VALUE_COEFF = 10, 11
HP_INDEX = dict(HP, demo_coeff=HP_DEMO_COEFF, demo_value_coeff=HP_DEMO_VALUE_COEFF)
# a third reserved field (the enumerator CADRE_HP_SUGGEST_COEFF), read by cadre_ppo_sug_loss only; set_hyper(suggest_coeff=)
HP_SUGGEST_COEFF = 12
# two more (the enumerators CADRE_HP_SIL_COEFF / CADRE_HP_SIL_VALUE_COEFF), read by cadre_ppo_sil_loss only;
# set_hyper(sil_coeff=, sil_value_coeff=)
HP_SIL_COEFF, HP_SIL_VALUE_COEFF = 13, 14
# the last field (the enumerator CADRE_HP_SMOOTH_COEFF), read by cadre_ppo_smooth_loss only; set_hyper(smooth_coeff=)
HP_SMOOTH_COEFF = 15
PPO_STATS_LR = 7      # CADRE_PPO_STATS_LR: field of head 0 of a stats row that cadre_grad_norms_hp fills with the step's lr

PPO_STATS_FIELDS = 8  # CADRE_PPO_STATS_FIELDS (include/cadre_hip.h): loss diagnostics per head before the gradient norms
BC_STATS_FIELDS = 6   # CADRE_BC_STATS_FIELDS: accuracy, NLL, entropy, |v - R|, weight sum, rows counted (means over inv_b)
AUX_STATS_FIELDS = 6  # CADRE_AUX_STATS_FIELDS: mean KL, max KL, mean |v - R|, mean entropy, mean (v - R)^2, rows counted
SUG_STATS_FIELDS = 4  # CADRE_SUG_STATS_FIELDS: marked rows, mean KL over the minibatch, max KL, mean p[prior's mode] over marked rows
SIL_STATS_FIELDS = 6  # CADRE_SIL_STATS_FIELDS: mean w, share w > 0, mean -lp, mean |R - v|, max w, rows counted (over the SIL rows)
SMOOTH_STATS_FIELDS = 4  # CADRE_SMOOTH_STATS_FIELDS: valid pairs, inv_bp sum |d|, max |d|, inv_bp sum d^2 (per head)
AM_STATS_FIELDS = 4   # CADRE_AM_STATS_FIELDS: share of properly masked rows, mean allowed bins, mean pressure, action bits OR-ed in
VTRACE_DIAG_FIELDS = 4  # CADRE_VTRACE_DIAG_FIELDS: mean ratio, share truncated, max |log ratio|, effective-sample share

# CADRE_RND_*: the curiosity state block (float64; mu [D], M2 [D], carry [N] from RND_HEAD on)
RND_N, RND_BETA, RND_EXT, RND_RHO_N, RND_RHO_MEAN, RND_RHO_M2, RND_SIGMA, RND_KEY, RND_CTR, RND_HEAD = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16
# CADRE_LAG_*: the cost-constraint state block (float64; LAG_STRIDE doubles per head)
LAG_LAMBDA, LAG_BUDGET, LAG_LR, LAG_MAX, LAG_J, LAG_SHARE, LAG_UPDATES, LAG_STRIDE = 0, 1, 2, 3, 4, 5, 6, 8
# CADRE_EMA_*: the weight-average state block (float64; dist2 [n_models] from EMA_HEAD on), the workgroups per model and the head
# of the scratch `work` (float64 [EMA_WORK_HEAD + n_models * EMA_GRID]), the bounds of n_models and of cadre_arena_mean's K
EMA_DECAY, EMA_WARMUP, EMA_COUNT, EMA_D, EMA_SKIPPED, EMA_HEAD = 0, 1, 2, 3, 4, 8
EMA_GRID, EMA_WORK_HEAD, EMA_MAX_MODELS, MEAN_MAX_SOURCES = 256, 2, 4096, 64
RS_SCALE, RS_CARRY = 6, 8 # CADRE_RS_SCALE / CADRE_RS_CARRY: the return-statistics block (count, mean, M2 per head first)

CAPTURE_MAX_RANGES = 65535        # CADRE_CAPTURE_MAX_RANGES
CAPTURE_BAD_RANGE = 2 ** 64 - 1   # CADRE_CAPTURE_BAD_RANGE: digest slot of a record the launch found malformed
DIGEST_K = 0x9E3779B97F4A7C15     # the digest's odd multiplier (include/cadre_hip.h)

N_CALLS = 0         # C-ABI calls checked so far (one kernel launch each, cadre_clip_adam_graph three): launch census


def check(rc, what):
    global N_CALLS
    N_CALLS += 1
    if rc != 0:
        msg = lib().cadre_last_error().decode() if rc < 0 else "hipError_t %d" % rc
        raise CadreHipError("%s failed: %s" % (what, msg))


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise CadreHipError("cadre_amd kernels need device (HIP) tensors; got a CPU tensor — there is no CPU path")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def capture_table(records, device):
    """Device range table of cadre_state_capture from host records [(src pointer, dst_off, bytes), ...] (int64 [n][3]).
    Everything the launch itself cannot report is refused here: bytes no multiple of 4 (state is fp32, fp64, int32 or
    int64), pointers or offsets off a 4-byte boundary, negative values, too many ranges."""
    if len(records) > CAPTURE_MAX_RANGES:
        raise CadreHipError("cadre_state_capture: %d ranges; at most %d per launch" % (len(records), CAPTURE_MAX_RANGES))
    for k, (src, off, nbytes) in enumerate(records):
        if nbytes < 0 or nbytes % 4 or off < 0 or off % 4 or src % 4 or (nbytes and not src):
            raise CadreHipError("cadre_state_capture: range %d (src 0x%x, dst_off %d, %d bytes) is not a run of 32-bit words: "
                                "bytes must be a multiple of 4, src and dst_off 4-byte aligned" % (k, src, off, nbytes))
    return torch.tensor([[int(v) for v in r] for r in records], dtype=torch.int64).reshape(len(records), 3).to(device)


def state_capture(table, n_ranges, staging, digests):
    """cadre_state_capture on the current stream: `table` from capture_table, `staging` a device byte buffer or None
    (digests only), `digests` a device int64 tensor of n_ranges slots (the uint64 digests' bit patterns)."""
    if digests.dtype != torch.int64 or digests.numel() < n_ranges or not digests.is_contiguous():
        raise CadreHipError("cadre_state_capture: digests must be a contiguous int64 tensor of at least %d slots" % n_ranges)
    if table.dtype != torch.int64 or table.numel() < 3 * n_ranges or not table.is_contiguous():
        raise CadreHipError("cadre_state_capture: the range table holds fewer than %d records" % n_ranges)
    check(lib().cadre_state_capture(ptr(table), n_ranges, ptr(staging), ptr(digests), stream()), "cadre_state_capture")


# Optional launch profiler (bench.py): when PROFILE is a list, every gemm launch is bracketed by
# HIP events recorded on the launch stream and appended as (key, flops, start, end, shape, bytes):
#   key   = (tile, a_mode, b_mode) for cadre_gemm_f32, ("bf16", tile, a_mode) for cadre_gemm_bf16
#   flops = algorithmic FLOPs of the launch, bytes = algorithmic HBM bytes (each operand once)
#   shape = (M, N, K, batch, split_k, seg_mode)
PROFILE = None


def _launch(name, fn, args, record):
    """check(fn(*args), name).  When PROFILE is a list and the stream is not capturing, the call is bracketed by two events and
    (key, flops, start, end, shape, bytes) is appended; record() -> (key, flops, shape, bytes), evaluated after the launch."""
    if PROFILE is None or torch.cuda.is_current_stream_capturing():
        check(fn(*args), name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(*args), name)
    e1.record()
    key, flops, shape, nbytes = record()
    PROFILE.append((key, flops, e0, e1, shape, nbytes))


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, a_mode=0, b_mode=0, scale=None, shift=None, resid=None, ldr=0,
         act=0, slope=0.01, batch=1, a_z=(1, 0, 0), b_z=(1, 0, 0), c_z=(1, 0, 0), s_z=(1, 0, 0), r_z=(1, 0, 0),
         conv=None, split_k=1, tile=0, bf16=False, flags=0, seg=None):
    """C = act((A . B^T) * scale + shift + resid).  *_z = (div, mod, stride) batch addressing.
    bf16=True: A/B are bfloat16 tensors (cadre_gemm_bf16); flags bit1/bit2: C / resid are bf16."""
    d = GemmDesc()
    d.A, d.B, d.C = ptr(A), ptr(B), ptr(Cout)
    d.scale, d.shift, d.resid = ptr(scale), ptr(shift), ptr(resid)
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.M, d.N, d.K, d.a_mode, d.b_mode, d.act, d.slope, d.batch = M, N, K, a_mode, b_mode, act, slope, batch
    (d.a_div, d.a_mod, d.a_str), (d.b_div, d.b_mod, d.b_str) = a_z, b_z
    (d.c_div, d.c_mod, d.c_str), (d.s_div, d.s_mod, d.s_str), (d.r_div, d.r_mod, d.r_str) = c_z, s_z, r_z
    if conv is not None:
        d.H, d.W, d.Cin, d.Ho, d.Wo, d.KH, d.KW, d.stride, d.pad = conv
    d.split_k, d.tile = split_k, tile
    d.flags = flags
    if seg is not None:                  # (mode, row_seg tensor, period, div)
        d.seg_mode, d.seg_period, d.seg_div = seg[0], seg[2], seg[3]
        d.row_seg = ptr(seg[1])
    fn = lib().cadre_gemm_bf16 if bf16 else lib().cadre_gemm_f32
    name = "cadre_gemm_bf16" if bf16 else "cadre_gemm_f32"

    def record():
        nb = max(1, batch)
        k_alg = conv[5] * conv[6] * conv[2] if conv is not None else K      # algorithmic K (the stems pad 196 -> 224 / 256)
        esz = 2 if bf16 else 4
        a_bytes = (M // (conv[3] * conv[4])) * conv[0] * conv[1] * conv[2] * esz if conv is not None else M * K * esz * nb
        c_esz = 2 if (flags & 2) else 4
        r_esz = 2 if (flags & 4) else 4
        nbytes = a_bytes + N * k_alg * esz * nb + M * N * c_esz * nb * max(1, split_k) + (M * N * r_esz * nb if resid is not None else 0)
        if bf16:
            key = ("bf16", lib().cadre_gemm_bf16_pick_tile(C.byref(d)), a_mode)
        else:
            key = (lib().cadre_gemm_pick_tile(C.byref(d)), a_mode, b_mode)
        return key, 2.0 * M * N * k_alg * nb, (M, N, K, nb, split_k, seg[0] if seg is not None else 0), nbytes
    _launch(name, fn, (C.byref(d), stream()), record)


def conv3x3_c64_bf16(x, w, scale, shift, resid, out, F, H, W, relu):
    """cadre_conv3x3_c64_bf16 (A/B build only) with the same profiling hook as gemm(): key ("bf16", 64, 2)."""
    if not has_ab_kernels():
        raise CadreHipError("cadre_conv3x3_c64_bf16 exists only in the A/B build (CADRE_BUILD_AB=1 python -m cadre_amd.build)")
    fn = lib().cadre_conv3x3_c64_bf16
    args = (ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(resid), ptr(out), F, H, W, relu, stream())

    def record():
        M = F * H * W
        nbytes = M * 64 * 2 * (3 if resid is not None else 2) + 64 * 576 * 2
        return ("bf16", 64, 2), 2.0 * M * 64 * 576, (M, 64, 576, 1, 1, 0), nbytes
    _launch("cadre_conv3x3_c64_bf16", fn, args, record)


def winograd_c64(x, u, scale, shift, resid, out, F, H, W, act):
    """cadre_winograd_c64 (fused Winograd F(2x2,3x3) of the fp32 64 -> 64 stage) with the profiling hook of gemm():
    key ("wino_c64", residual); FLOPs = the EXECUTED ones (16 planes x tiles x 64 x 64)."""
    fn = lib().cadre_winograd_c64
    args = (ptr(x), ptr(u), ptr(scale), ptr(shift), ptr(resid), ptr(out), F, H, W, act, stream())

    def record():
        T = F * ((H + 1) // 2) * ((W + 1) // 2)
        nbytes = F * H * W * 64 * 4 * (3 if resid is not None else 2) + 16 * 64 * 64 * 4
        return ("wino_c64", resid is not None), 2.0 * 16 * T * 64 * 64, (T, 64, 64 * 16, 1, 1, 0), nbytes
    _launch("cadre_winograd_c64", fn, args, record)


def winograd_fused(x, V, u_frag, scale, shift, resid, out, F, H, W, Cin, N, act, m):
    """cadre_winograd_in_frag + cadre_winograd_gemm_out (Winograd F(m x m, 3x3): the plane products and the inverse transform in one
    kernel, csrc/winograd_fused.hip).  Profiling key ("wgo", m, ntb) on the product kernel: wino_gemm_out_kernel<m, ntb>; FLOPs = the EXECUTED
    ones ((m+2)^2 planes x tiles x Cin x N), bytes = V read once + the output written (+ the residual read) + U."""
    L = lib()
    check(L.cadre_winograd_in_frag(ptr(x), ptr(V), F, H, W, Cin, m, stream()), "cadre_winograd_in_frag")
    fn = L.cadre_winograd_gemm_out
    args = (ptr(V), ptr(u_frag), ptr(scale), ptr(shift), ptr(resid), ptr(out), F, H, W, Cin, N, act, m, stream())

    def record():
        P, T = (m + 2) ** 2, F * -(-H // m) * -(-W // m)
        nbytes = (P * T * Cin + P * N * Cin + F * H * W * N * (2 if resid is not None else 1)) * 4
        return ("wgo", m, int(L.cadre_winograd_fused_ntb(T, N))), 2.0 * P * T * Cin * N, (T, N, Cin * P, 1, 1, 0), nbytes
    _launch("cadre_winograd_gemm_out", fn, args, record)


def conv3x3_s2(x, w_s2, scale, shift, out, F, H, W, Cin, N, act):
    """cadre_conv3x3_s2 (3x3 / s2 / p1 on bf16 NHWC: four parity-plane windows in LDS); profiling key ("s2", npw):
    conv3x3_s2_kernel<npw>, npw = window pieces per wave (9 for output rows of <= 31 pixels, else 10)."""
    fn = lib().cadre_conv3x3_s2
    args = (ptr(x), ptr(w_s2), ptr(scale), ptr(shift), ptr(out), F, H, W, Cin, N, act, stream())

    def record():
        M = F * (H // 2) * (W // 2)
        nbytes = F * H * W * Cin * 2 + N * 9 * Cin * 2 + M * N * 2
        npw = 9 if (256 + W // 2 + 1 + 7) // 8 <= 36 else 10
        return ("s2", npw), 2.0 * M * N * 9 * Cin, (M, N, 9 * Cin, 1, 1, 0), nbytes
    _launch("cadre_conv3x3_s2", fn, args, record)


def conv3x3_s1x(x, x2, w_s1x, shift, out, F, H, W, C1, Cd, N, act):
    """cadre_conv3x3_s1x (3x3 / s1 conv + the block's 1x1 / s2 shortcut as extra k-tiles, one accumulation); profiling key
    ("s1x", nps, nstg): conv3x3_s1x_kernel<nps, nstg>, nps = stride-1 window pieces per wave (9 / 10 / 11 by map width), nstg =
    weight stages (2; CADRE_S1X_STAGES=3 selects the symmetric-issue form)."""
    fn = lib().cadre_conv3x3_s1x
    args = (ptr(x), ptr(x2), ptr(w_s1x), ptr(shift), ptr(out), F, H, W, C1, Cd, N, act, stream())

    def record():
        M = F * H * W
        nbytes = (M * C1 + M * Cd + N * (9 * C1 + Cd) + M * N) * 2          # (the shortcut reads one pixel in four of x2)
        pa = ((256 + 2 * W + 2 + 7) // 8 * 8) // 8
        nps = 9 if pa <= 36 else (10 if pa <= 40 else 11)
        nstg = int(lib().cadre_conv3x3_s1x_stages(W, N))       # (what the library launches: a request for 3 stages falls back to 2 where they do not fit)
        return ("s1x", nps, nstg), 2.0 * M * N * (9 * C1 + Cd), (M, N, 9 * C1 + Cd, 1, 1, 0), nbytes
    _launch("cadre_conv3x3_s1x", fn, args, record)


def gemm_bf16_w128(A, B_frag, slabs, M, N, K, lda, ldc, split_k):
    """cadre_gemm_bf16_w128 (dense bf16 split-K product, 128 x 128 wave tile, B streamed to registers in fragment order); profiling
    key ("gw128",): gemm_bf16_w128_kernel."""
    fn = lib().cadre_gemm_bf16_w128
    args = (ptr(A), ptr(B_frag), ptr(slabs), M, N, K, lda, ldc, split_k, stream())

    def record():
        nbytes = (M * K + N * K) * 2 + M * N * 4 * split_k
        return ("gw128",), 2.0 * M * N * K, (M, N, K, 1, split_k, 0), nbytes
    _launch("cadre_gemm_bf16_w128", fn, args, record)


def w128_shape(W, N):
    """(MW, NPW) template arguments cadre_conv3x3_w128 picks (conv3x3_w128.hip w128_pick) — the profiling key / kernel name."""
    mw = 2 if N % 256 == 0 else 4
    need = (128 * mw + 2 * W + 2 + 31) // 32
    if mw == 2:
        return mw, (9 if need <= 9 else (10 if need <= 10 else 11))
    return mw, (17 if need <= 17 else 19)


def conv3x3_w128(x, w_frag, shift, resid, out, F, H, W, Cin, N, act):
    """cadre_conv3x3_w128 (3x3 / s1 window conv, 128 x 128 wave tile, weights streamed to registers); profiling key
    ("w128", mw, npw, residual): conv3x3_w128_kernel<mw, npw, residual>.  A/B build only."""
    if not has_ab_kernels():
        raise CadreHipError("cadre_conv3x3_w128 exists only in the A/B build (CADRE_BUILD_AB=1 python -m cadre_amd.build)")
    fn = lib().cadre_conv3x3_w128
    args = (ptr(x), ptr(w_frag), None, ptr(shift), ptr(resid), ptr(out), F, H, W, Cin, N, act, stream())

    def record():
        M = F * H * W
        nbytes = (M * Cin + N * 9 * Cin + M * N * (2 if resid is not None else 1)) * 2
        mw, npw = w128_shape(W, N)
        return ("w128", mw, npw, resid is not None), 2.0 * M * N * 9 * Cin, (M, N, 9 * Cin, 1, 1, 0), nbytes
    _launch("cadre_conv3x3_w128", fn, args, record)


def conv3x3_ring(x, w_ring, scale, shift, resid, out, F, H, W, Cin, N, act):
    """cadre_conv3x3_ring (3x3 / s1 / p1, each pixel through LDS once per channel chunk); profiling key
    ("ring", bf16, ntile, res, out_bf16, WVM, pp, G): pp 0 = conv3x3_ring_kernel<bf16, ntile, res, out_bf16, WVM>,
    pp 1, G 0 = conv3x3_ring_pp_kernel<bf16, ntile, res, out_bf16, false> (the 8-wave ping-pong kernel), G > 0 =
    conv3x3_ring_pp2_kernel<ntile, res, out_bf16, G> (G k-tiles per ping-pong slot)."""
    bf = x.dtype == torch.bfloat16
    flags = (1 if bf else 0) | (2 if out.dtype == torch.bfloat16 else 0) | (4 if (resid is not None and resid.dtype == torch.bfloat16) else 0)
    fn = lib().cadre_conv3x3_ring
    args = (ptr(x), ptr(w_ring), ptr(scale), ptr(shift), ptr(resid), ptr(out), F, H, W, Cin, N, act, flags, stream())

    def record():
        M, esz = F * H * W, (2 if bf else 4)
        nbytes = M * Cin * esz + N * 9 * Cin * esz + M * N * out.element_size() + (M * N * resid.element_size() if resid is not None else 0)
        code = lib().cadre_conv3x3_ring_ntile(F, H, W, Cin, N, 1 if bf else 0)      # ntile + 1000 * WVM + 100000 * ping-pong + 1000000 * G
        res = 0 if resid is None else (2 if resid.dtype == torch.bfloat16 else 1)
        key = ("ring", bf, code % 1000, res, out.dtype == torch.bfloat16, code // 1000 % 100, code // 100000 % 10, code // 1000000)
        return key, 2.0 * M * N * 9 * Cin, (M, N, 9 * Cin, 1, 1, 0), nbytes
    _launch("cadre_conv3x3_ring", fn, args, record)


def deconv3x3_s2(x, x_zstride, w, scale, shift, out, Z, F, H, W, Cin, Cout, oph, opw, act=0, slope=0.01):
    """cadre_deconv3x3_s2 (ConvTranspose2d 3x3 / s2 / p1 as four parity-class implicit GEMMs, csrc/deconv.hip) with the profiling
    hook of gemm(): key ("deconv", Cin, Cout); FLOPs = the EXECUTED ones, 9 taps x Cin x Cout per input position (a tap the
    map's last row / column does not have is multiplied as zeros)."""
    fn = lib().cadre_deconv3x3_s2
    args = (ptr(x), x_zstride, ptr(w), ptr(scale), ptr(shift), ptr(out), Z, F, H, W, Cin, Cout, oph, opw, act, slope, stream())

    def record():
        Ho, Wo = 2 * H - 1 + oph, 2 * W - 1 + opw
        nbytes = (F * H * W * Cin * (Z if x_zstride else 1) + Z * 9 * Cin * Cout + Z * F * Ho * Wo * Cout) * 4
        return ("deconv", Cin, Cout), 2.0 * Z * F * H * W * 9 * Cin * Cout, (F * H * W, Cout, 9 * Cin, Z, 1, 0), nbytes
    _launch("cadre_deconv3x3_s2", fn, args, record)


def deconv3x3_s2_out(x, w, bias, logits, cls, sig, F, H, W, Cout, oph=1, opw=1):
    """cadre_deconv3x3_s2_out (last decoder level, 32 -> Cout <= 8 on the vector ALU); logits / cls / sig: a tensor, or None when
    that output is not wanted.  Profiling key ("deconv_out", Cout)."""
    fn = lib().cadre_deconv3x3_s2_out
    args = (ptr(x), ptr(w), ptr(bias), ptr(logits), ptr(cls), ptr(sig), F, H, W, Cout, oph, opw, stream())

    def record():
        Ho, Wo = 2 * H - 1 + oph, 2 * W - 1 + opw
        nbytes = F * H * W * 32 * 4 + F * Ho * Wo * ((Cout * 4 if logits is not None else 0) + (1 if cls is not None else 0) + (4 if sig is not None else 0))
        return ("deconv_out", Cout), 2.0 * F * H * W * 9 * 32 * Cout, (F * H * W, Cout, 9 * 32, 1, 1, 0), nbytes
    _launch("cadre_deconv3x3_s2_out", fn, args, record)
