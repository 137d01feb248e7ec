"""ctypes binding of the C ABI in include/trlx_t5_amd.h (libtrlx_t5_amd.so, built in-tree
for gfx950 by `make -C trlx-t5_amd/csrc` / `__graft_entry__.build()`).

There is no fallback: if the shared library is missing or fails to load, every entry
point raises.  torch is imported first so the HIP runtime the library links against
(libamdhip64.so.7) resolves to the one torch already loaded — the library then launches
on torch's streams directly.
"""
import contextlib
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# TRLX_T5_AMD_LIB: another build of the same library (A/B tooling only, e.g. scripts/ab_rows.sh)
LIB_PATH = os.environ.get("TRLX_T5_AMD_LIB") or os.path.join(_HERE, "libtrlx_t5_amd.so")

F32, BF16, I64 = 0, 1, 2
ABI_VERSION = 2
MOMENT_SLOTS = 4
SPLIT_MOMENT_SLOTS = 8  # split-beta record {Σ A0, Σ A0², n, Σ Ak, Σ A0·Ak, Σ Ak², Σ mask, 0}
PPO_STATS = 13
PPO_PARTIAL_SLOTS = 16

_c_vp, _c_i64, _c_int, _c_f, _c_d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double


class IlqlArgs(ctypes.Structure):
    """Mirror of trlx_ilql_args (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("dtype", _c_int), ("nq", _c_int),
        ("B", _c_i64), ("L", _c_i64), ("A", _c_i64), ("V", _c_i64),
        ("logits", _c_vp), ("logits_sb", _c_i64), ("logits_st", _c_i64),
        ("q", _c_vp * 2), ("q_sb", _c_i64 * 2), ("q_st", _c_i64 * 2),
        ("tq", _c_vp * 2), ("tq_sb", _c_i64 * 2), ("tq_st", _c_i64 * 2),
        ("input_ids", _c_vp), ("attention_mask", _c_vp), ("actions_ixs", _c_vp), ("dones", _c_vp),
        ("rewards", _c_vp), ("rewards_dtype", _c_int),
        ("vs", _c_vp), ("vs_dtype", _c_int),
        ("tau", _c_f), ("gamma", _c_f), ("cql_scale", _c_f), ("awac_scale", _c_f),
        ("dlogits", _c_vp), ("dlogits_sb", _c_i64), ("dlogits_st", _c_i64),
        ("dq", _c_vp * 2), ("dq_sb", _c_i64 * 2), ("dq_st", _c_i64 * 2),
        ("dvs", _c_vp), ("losses", _c_vp), ("workspace", _c_vp),
        ("tq_gathered", _c_int),
    ]


class IlqlTqArgs(ctypes.Structure):
    """Mirror of trlx_ilql_tq_args (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("dtype", _c_int), ("nh", _c_int),
        ("B", _c_i64), ("L", _c_i64), ("A", _c_i64), ("K", _c_i64), ("V", _c_i64),
        ("z", _c_vp * 2), ("z_sb", _c_i64 * 2), ("z_st", _c_i64 * 2),
        ("w2", _c_vp * 2), ("w2_ld", _c_i64 * 2),
        ("b2", _c_vp * 2),
        ("input_ids", _c_vp), ("actions_ixs", _c_vp),
        ("out", _c_vp * 2),
    ]


class PpoSampleProcArgs(ctypes.Structure):
    """Mirror of TrlxPpoSampleProcArgs (include/trlx_t5_amd.h): the plain step, the record block
    (ref_logits NULL = none), the processor block."""
    _fields_ = [
        ("logits", _c_vp), ("ld_logits", _c_i64), ("B", _c_i64), ("V", _c_i64),
        ("dtype", _c_int), ("top_k", _c_int), ("temperature", _c_f), ("top_p", _c_f),
        ("min_tokens_to_keep", _c_int), ("score_finished", _c_int),
        ("cur_len", _c_i64), ("min_length", _c_i64), ("eos_token_id", _c_i64), ("pad_token_id", _c_i64),
        ("u", _c_vp), ("out_ids", _c_vp), ("out_logprobs", _c_vp), ("out_min_kept", _c_vp),
        ("out_kept_count", _c_vp), ("unfinished", _c_vp),
        ("ref_logits", _c_vp), ("ld_ref", _c_i64), ("t", _c_i64), ("T", _c_i64),
        ("tokens", _c_vp), ("ld_tokens", _c_i64), ("logprobs", _c_vp), ("ld_logprobs", _c_i64),
        ("ref_logprobs", _c_vp), ("ld_ref_logprobs", _c_i64), ("values", _c_vp), ("ld_values", _c_i64),
        ("step_values", _c_vp), ("lengths", _c_vp), ("ref_dtype", _c_int), ("values_dtype", _c_int),
        ("repetition_penalty", _c_f), ("no_repeat_ngram_size", _c_int), ("forced_token_id", _c_i64),
        ("prefix0", _c_vp), ("prefix0_ld", _c_i64), ("prefix0_len", _c_i64),
        ("prefix1", _c_vp), ("prefix1_ld", _c_i64), ("prefix1_len", _c_i64),
        ("bad_words", _c_vp), ("bad_words_offsets", _c_vp), ("bad_words_host", _c_vp),
        ("bad_words_offsets_host", _c_vp), ("n_bad_words", _c_i64),
    ]


class PpoSampleDevArgs(ctypes.Structure):
    """Mirror of TrlxPpoSampleDevArgs (include/trlx_t5_amd.h): the device-clock step's extra block."""
    _fields_ = [("clock", _c_vp), ("forced_bos_token_id", _c_i64), ("forced_eos_token_id", _c_i64),
                ("max_length", _c_i64), ("u_ld", _c_i64)]


# the decode clock record (include/trlx_t5_amd.h): int64 words
CLOCK_T, CLOCK_CAP, CLOCK_CUR_LEN0, CLOCK_OVERRUN, CLOCK_WORDS = 0, 1, 2, 3, 8

T5_ATTN_SELF, T5_ATTN_CROSS = 0, 1


class T5DecodeAttnArgs(ctypes.Structure):
    """Mirror of TrlxT5DecodeAttnArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("q", _c_vp), ("ldq", _c_i64), ("k_new", _c_vp), ("ldk", _c_i64), ("v_new", _c_vp), ("ldv", _c_i64),
        ("k", _c_vp), ("v", _c_vp), ("bias_by_distance", _c_vp), ("key_mask", _c_vp), ("out", _c_vp),
        ("B", _c_i64), ("n_heads", _c_i64), ("d_kv", _c_i64), ("max_len", _c_i64), ("t", _c_i64),
        ("dtype", _c_int), ("mode", _c_int),
    ]


class T5CrossKvQuantArgs(ctypes.Structure):
    """Mirror of TrlxT5CrossKvQuantArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("k", _c_vp), ("k_stride_b", _c_i64), ("k_stride_h", _c_i64), ("k_stride_s", _c_i64),
        ("v", _c_vp), ("v_stride_b", _c_i64), ("v_stride_h", _c_i64), ("v_stride_s", _c_i64),
        ("key_mask", _c_vp), ("k8", _c_vp), ("v8", _c_vp), ("k_scale", _c_vp), ("v_scale", _c_vp),
        ("B", _c_i64), ("n_heads", _c_i64), ("S", _c_i64), ("d_kv", _c_i64),
    ]


class T5DecodeAttnGroupArgs(ctypes.Structure):
    """Mirror of TrlxT5DecodeAttnGroupArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("q", _c_vp), ("ldq", _c_i64),
        ("k", _c_vp), ("k_stride_p", _c_i64), ("k_stride_h", _c_i64), ("k_stride_s", _c_i64),
        ("v", _c_vp), ("v_stride_p", _c_i64), ("v_stride_h", _c_i64), ("v_stride_s", _c_i64),
        ("key_mask", _c_vp), ("live", _c_vp), ("out", _c_vp),
        ("P", _c_i64), ("G", _c_i64), ("n_heads", _c_i64), ("d_kv", _c_i64), ("S", _c_i64), ("dtype", _c_int),
    ]


class T5DecodeAttnSplitGeometry(ctypes.Structure):
    """Mirror of TrlxT5DecodeAttnSplitGeometry (include/trlx_t5_amd.h)."""
    _fields_ = [("NG", _c_i64), ("C", _c_i64), ("ranges", _c_i64), ("tile", _c_i64), ("max_splits", _c_i64)]


class T5DecodeEmbedArgs(ctypes.Structure):
    """Mirror of TrlxT5DecodeEmbedArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("weight", _c_vp), ("ld_w", _c_i64), ("tokens", _c_vp), ("ld_tokens", _c_i64), ("norm_w", _c_vp),
        ("h", _c_vp), ("ld_h", _c_i64), ("y", _c_vp), ("ld_y", _c_i64),
        ("B", _c_i64), ("D", _c_i64), ("V", _c_i64), ("T", _c_i64), ("t", _c_i64), ("start_token_id", _c_i64),
        ("eps", _c_f), ("dtype", _c_int),
    ]


class T5AttentionArgs(ctypes.Structure):
    """Mirror of TrlxT5AttentionArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("q", _c_vp), ("q_stride_b", _c_i64), ("q_stride_t", _c_i64), ("q_stride_h", _c_i64),
        ("k", _c_vp), ("k_stride_b", _c_i64), ("k_stride_t", _c_i64), ("k_stride_h", _c_i64),
        ("v", _c_vp), ("v_stride_b", _c_i64), ("v_stride_t", _c_i64), ("v_stride_h", _c_i64),
        ("out", _c_vp), ("o_stride_b", _c_i64), ("o_stride_t", _c_i64), ("o_stride_h", _c_i64),
        ("bias_by_offset", _c_vp), ("key_mask", _c_vp),
        ("B", _c_i64), ("n_heads", _c_i64), ("d_kv", _c_i64), ("Tq", _c_i64), ("S", _c_i64),
        ("dtype", _c_int), ("causal", _c_int),
    ]


class T5AttentionBwdArgs(ctypes.Structure):
    """Mirror of TrlxT5AttentionBwdArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("q", _c_vp), ("q_stride_b", _c_i64), ("q_stride_t", _c_i64), ("q_stride_h", _c_i64),
        ("k", _c_vp), ("k_stride_b", _c_i64), ("k_stride_t", _c_i64), ("k_stride_h", _c_i64),
        ("v", _c_vp), ("v_stride_b", _c_i64), ("v_stride_t", _c_i64), ("v_stride_h", _c_i64),
        ("out", _c_vp), ("o_stride_b", _c_i64), ("o_stride_t", _c_i64), ("o_stride_h", _c_i64),
        ("dout", _c_vp), ("do_stride_b", _c_i64), ("do_stride_t", _c_i64), ("do_stride_h", _c_i64),
        ("dq", _c_vp), ("dq_stride_b", _c_i64), ("dq_stride_t", _c_i64), ("dq_stride_h", _c_i64),
        ("dk", _c_vp), ("dk_stride_b", _c_i64), ("dk_stride_t", _c_i64), ("dk_stride_h", _c_i64),
        ("dv", _c_vp), ("dv_stride_b", _c_i64), ("dv_stride_t", _c_i64), ("dv_stride_h", _c_i64),
        ("lse", _c_vp), ("bias_by_offset", _c_vp), ("key_mask", _c_vp), ("dbias", _c_vp),
        ("workspace", _c_vp), ("workspace_bytes", _c_i64),
        ("B", _c_i64), ("n_heads", _c_i64), ("d_kv", _c_i64), ("Tq", _c_i64), ("S", _c_i64),
        ("dtype", _c_int), ("causal", _c_int),
    ]


T5_ACT_RELU, T5_ACT_GELU_NEW, T5_ACT_SILU = 0, 1, 2


class T5FfActArgs(ctypes.Structure):
    """Mirror of TrlxT5FfActArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("u", _c_vp), ("ld_u", _c_i64), ("v", _c_vp), ("ld_v", _c_i64), ("out", _c_vp), ("ld_out", _c_i64),
        ("dy", _c_vp), ("ld_dy", _c_i64), ("du", _c_vp), ("ld_du", _c_i64), ("dv", _c_vp), ("ld_dv", _c_i64),
        ("N", _c_i64), ("F", _c_i64), ("dtype", _c_int), ("act", _c_int),
    ]


class T5RmsNormArgs(ctypes.Structure):
    """Mirror of TrlxT5RmsNormArgs (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("x", _c_vp), ("ld_x", _c_i64), ("residual", _c_vp), ("ld_residual", _c_i64), ("h", _c_vp), ("ld_h", _c_i64),
        ("y", _c_vp), ("ld_y", _c_i64), ("dy", _c_vp), ("ld_dy", _c_i64), ("dh_in", _c_vp), ("ld_dh_in", _c_i64),
        ("dh", _c_vp), ("ld_dh", _c_i64), ("w", _c_vp), ("dw", _c_vp), ("rstd", _c_vp), ("ws", _c_vp),
        ("ws_bytes", _c_i64), ("N", _c_i64), ("D", _c_i64), ("eps", _c_f), ("dtype", _c_int),
    ]


class T5RmsNormGeometry(ctypes.Structure):
    """Mirror of TrlxT5RmsNormGeometry (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("vec_bf16", _c_int), ("vec_f32", _c_int), ("threads", _c_int), ("max_partials", _c_int), ("max_d", _c_int),
        ("reg_max_d", _c_int), ("wave_row_max_d", _c_int), ("n_breaks", _c_int), ("d_breaks", _c_int * 8),
        ("rows_per_block", _c_int), ("reserved", _c_int), ("row_blocks", _c_i64), ("partials", _c_i64),
        ("ws_bytes", _c_i64),
    ]


T5_ACT_NONE = -1


class T5DecodeLinearArgs(ctypes.Structure):
    """Mirror of trlx_t5_decode_linear_args (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("x", _c_vp), ("ld_x", _c_i64), ("weight", _c_vp), ("ld_w", _c_i64), ("norm_weight", _c_vp),
        ("residual", _c_vp), ("ld_residual", _c_i64), ("out", _c_vp), ("ld_out", _c_i64),
        ("M", _c_i64), ("K", _c_i64), ("N", _c_i64), ("eps", _c_f), ("dtype", _c_int), ("act", _c_int), ("gated", _c_int),
    ]


class T5DecodeLinearGeometry(ctypes.Structure):
    """Mirror of TrlxT5DecodeLinearGeometry (include/trlx_t5_amd.h)."""
    _fields_ = [(n, _c_int) for n in ("threads", "cols_per_block", "rows_per_tile", "k_per_chunk", "chunks_per_wave_turn",
                                      "max_row_tiles", "max_k", "norm_max_k", "norm_wave_row_max_k", "reserved")]


class T5DecodeLinearRowsArgs(ctypes.Structure):
    """Mirror of trlx_t5_decode_linear_rows_args (include/trlx_t5_amd.h)."""
    _fields_ = T5DecodeLinearArgs._fields_ + [("live", _c_vp), ("reserved", _c_i64)]


class T5DecodeLinearRowsGeometry(ctypes.Structure):
    """Mirror of TrlxT5DecodeLinearRowsGeometry (include/trlx_t5_amd.h)."""
    _fields_ = [(n, _c_int) for n in ("threads", "cols_per_block", "rows_per_tile", "rows_per_block", "max_m_live", "reserved")]


POLYAK_MAX_TENSORS = 16
ADAMW_MAX_TENSORS = 32
ADAMW_CHUNK = 8192  # elements of one tensor per workgroup


class AdamwArgs(ctypes.Structure):
    """Mirror of trlx_adamw_args (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("p_dtype", _c_int), ("g_dtype", _c_int), ("count", _c_i64),
        ("p", ctypes.POINTER(_c_vp)), ("g", ctypes.POINTER(_c_vp)), ("m", ctypes.POINTER(_c_vp)),
        ("v", ctypes.POINTER(_c_vp)), ("master", ctypes.POINTER(_c_vp)), ("target", ctypes.POINTER(_c_vp)),
        ("numel", ctypes.POINTER(_c_i64)),
        ("step", _c_i64), ("lr", _c_d), ("beta1", _c_d), ("beta2", _c_d), ("eps", _c_d), ("weight_decay", _c_d),
        ("alpha", _c_d), ("lr_table", _c_vp), ("n_lr", _c_i64),
    ]


class GradNormRecord(ctypes.Structure):
    """Mirror of trlx_grad_norm_record (include/trlx_t5_amd.h): 32 bytes on the device."""
    _fields_ = [("norm", _c_f), ("coef", _c_f), ("nonfinite", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("sumsq", _c_d), ("reserved", _c_i64)]


class GradNormArgs(ctypes.Structure):
    """Mirror of trlx_grad_norm_args (include/trlx_t5_amd.h)."""
    _fields_ = [
        ("count", _c_i64), ("g", ctypes.POINTER(_c_vp)), ("g_dtype", ctypes.POINTER(_c_int)),
        ("numel", ctypes.POINTER(_c_i64)), ("max_norm", _c_d), ("record", _c_vp), ("workspace", _c_vp),
        ("workspace_bytes", _c_i64), ("scale_in_place", _c_int),
    ]


class AdamwSched(ctypes.Structure):
    """Mirror of trlx_adamw_sched (include/trlx_t5_amd.h): 96 bytes on the device."""
    _fields_ = [("step", _c_i64), ("skipped", _c_i64), ("apply", ctypes.c_int32), ("sync", ctypes.c_int32),
                ("decay", _c_f), ("w1", _c_f), ("b2", _c_f), ("w2", _c_f), ("neg_step", _c_f), ("sqrt_bc2", _c_f),
                ("eps", _c_f), ("alpha", _c_f), ("beta", _c_f), ("pad", _c_f), ("lr", _c_d), ("reserved", _c_i64 * 3)]


class AdamwAdvanceArgs(ctypes.Structure):
    """Mirror of trlx_adamw_advance_args (include/trlx_t5_amd.h)."""
    _fields_ = [("sched", _c_vp), ("beta1", _c_d), ("beta2", _c_d), ("eps", _c_d), ("weight_decay", _c_d),
                ("alpha", _c_d), ("lr_table", _c_vp), ("n_lr", _c_i64), ("sync_every", _c_i64),
                ("grad_record", _c_vp), ("skip_nonfinite", _c_int)]


_ilql_p = ctypes.POINTER(IlqlArgs)
_ilql_tq_p = ctypes.POINTER(IlqlTqArgs)
_adamw_p = ctypes.POINTER(AdamwArgs)
_grad_norm_p = ctypes.POINTER(GradNormArgs)

CTL_SLOTS = 16
(CTL_MEAN, CTL_VAR, CTL_STD, CTL_COUNT, CTL_REF_MEAN, CTL_REF_STD, CTL_REF_SET, CTL_KL_COEF, CTL_BATCH_MEAN,
 CTL_BATCH_STD, CTL_KL_UPDATES, CTL_LAST_KL) = range(12)
SCALE_NONE, SCALE_RUNNING, SCALE_REF = 0, 1, 2


class ScoreCtl(ctypes.Structure):
    """Mirror of trlx_score_ctl (include/trlx_t5_amd.h)."""
    _fields_ = [("state_in", _c_vp), ("state_out", _c_vp), ("global_moments", _c_vp), ("scale_mode", _c_int),
                ("cliprange_reward", _c_f)]


class KlCtl(ctypes.Structure):
    """Mirror of trlx_kl_ctl (include/trlx_t5_amd.h)."""
    _fields_ = [("state", _c_vp), ("adaptive", _c_int), ("target", _c_d), ("horizon", _c_d), ("n_steps", _c_i64)]


class GaeSplitArgs(ctypes.Structure):
    """Mirror of trlx_gae_split_args (include/trlx_t5_amd.h)."""
    _fields_ = [("B", _c_i64), ("T", _c_i64), ("lp", _c_vp), ("ref_lp", _c_vp), ("values", _c_vp), ("v_dtype", _c_int),
                ("scores", _c_vp), ("lengths", _c_vp), ("mask", _c_vp), ("ctl", ctypes.POINTER(ScoreCtl)),
                ("kl_coef", _c_f), ("gamma", _c_d), ("lam", _c_d), ("adv0", _c_vp), ("adv_kl", _c_vp),
                ("rew_kl", _c_vp), ("rew_score", _c_vp), ("stats8", _c_vp), ("mom_lag", _c_int),
                ("workspace", _c_vp)]


_score_ctl_p = ctypes.POINTER(ScoreCtl)
_kl_ctl_p = ctypes.POINTER(KlCtl)
_gae_split_p = ctypes.POINTER(GaeSplitArgs)

# name -> (restype, argtypes)   (must match include/trlx_t5_amd.h exactly)
SIGNATURES = {
    "trlx_abi_version": (_c_int, []),
    "trlx_last_error": (ctypes.c_char_p, []),
    "trlx_set_tuning": (_c_int, [ctypes.c_char_p, _c_i64]),
    "trlx_lsm_gather_fwd": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                     _c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    "trlx_ragged_order_bytes": (_c_i64, [_c_i64, _c_i64]),
    "trlx_lsm_gather_fwd_ragged": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                            _c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp]),
    "trlx_lsm_gather_bwd": (_c_int, [_c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp,
                                     _c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp, _c_i64, _c_i64, _c_vp]),
    "trlx_kl_penalty_rewards": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_f, _c_vp, _c_vp,
                                         _c_vp, _c_int, _c_vp]),
    "trlx_gae_num_blocks": (_c_i64, [_c_i64, _c_i64]),
    "trlx_gae_scan": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_d, _c_d, _c_vp, _c_vp,
                               _c_f, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp,
                               _c_vp, _c_vp, _c_vp]),
    "trlx_moments_num_blocks": (_c_i64, [_c_i64]),
    "trlx_moments_partial": (_c_int, [_c_vp, _c_int, _c_i64, _c_vp, _c_vp]),
    "trlx_moments_finalize": (_c_int, [_c_vp, _c_i64, _c_vp, _c_vp]),
    "trlx_whiten_apply": (_c_int, [_c_vp, _c_int, _c_i64, _c_vp, _c_int, _c_int, _c_vp, _c_int, _c_vp]),
    "trlx_ppo_policy_fused": (_c_int, [_c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp,
                                       _c_i64, _c_i64, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                       _c_d, _c_f, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp]),
    "trlx_ppo_loss_num_blocks": (_c_i64, [_c_i64]),
    "trlx_ppo_loss_elem": (_c_int, [_c_i64, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_int,
                                    _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_d,
                                    _c_f, _c_f, _c_f, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp,
                                    _c_vp]),
    "trlx_ppo_loss_finalize": (_c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_d, _c_f, _c_vp, _c_vp, _c_vp]),
    "trlx_scale_by": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_vp, _c_vp]),
    "trlx_ppo_workspace_bytes": (_c_i64, [_c_i64, _c_i64]),
    "trlx_ppo_rollout_gae": (_c_int, [_c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_f, _c_d,
                                      _c_d, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    "trlx_ppo_loss_rows": (_c_int, [_c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64, _c_i64,
                                    _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_int,
                                    _c_vp, _c_int, _c_f, _c_f, _c_f, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp,
                                    _c_vp]),
    "trlx_ppo_rollout_loss": (_c_int, [_c_i64, _c_i64, _c_vp, _c_f, _c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_ppo_experience_fused": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                           _c_vp, _c_i64, _c_i64, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_f,
                                           _c_d, _c_d, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp,
                                           _c_vp, _c_vp]),
    "trlx_ppo_loss_fused": (_c_int, [_c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                     _c_i64, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int,
                                     _c_vp, _c_int, _c_vp, _c_int, _c_f, _c_f, _c_f, _c_vp, _c_vp, _c_i64,
                                     _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_lmhead_workspace_bytes": (_c_i64, [_c_i64, _c_i64]),
    "trlx_lmhead_loss_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "trlx_ppo_loss_from_hidden": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp,
                                           _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp,
                                           _c_int, _c_f, _c_f, _c_f, _c_vp, _c_vp, _c_i64, _c_int, _c_vp,
                                           _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp]),
    "trlx_lmhead_loss_bwd_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "trlx_ppo_loss_from_hidden_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "trlx_ppo_loss_from_hidden_plan": (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64]),
    "trlx_ppo_loss_from_hidden_split": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp,
                                                 _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp,
                                                 _c_f, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_vp,
                                                 _c_int, _c_f, _c_f, _c_f, _c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_int,
                                                 _c_i64, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp]),
    "trlx_lmhead_logprobs_fwd_saved": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                                _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_lmhead_logprobs_bwd": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp,
                                          _c_int, _c_vp, _c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_int, _c_i64, _c_vp,
                                          _c_vp]),
    "trlx_lmhead_savep_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "trlx_lmhead_logprobs_fwd_ex": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                             _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_lmhead_logprobs_bwd_ex": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                             _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_int,
                                             _c_i64, _c_vp, _c_vp, _c_vp]),
    "trlx_lmhead_logprobs_fwd_ex2": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                              _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp,
                                              ctypes.POINTER(_c_i64), _c_vp]),
    "trlx_lmhead_logprobs_bwd_ex2": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                              _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_i64, _c_int, _c_vp, _c_int,
                                              _c_i64, _c_vp, _c_vp, _c_i64, _c_vp]),
    "trlx_lmhead_set_variant": (_c_int, [_c_int]),
    "trlx_lmhead_logprobs": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp,
                                      _c_int, _c_vp, _c_vp, _c_vp]),
    "trlx_lmhead_logprobs_ragged": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                             _c_vp, _c_i64, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    "trlx_ilql_sample": (_c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_vp, _c_i64, _c_int, _c_vp, _c_vp, _c_i64, _c_vp,
                                  _c_i64, _c_i64, _c_f, _c_int, _c_f, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp]),
    "trlx_ppo_sample": (_c_int, [_c_vp, _c_i64, _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_f, _c_int, _c_i64, _c_i64,
                                 _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_ppo_sample_record": (_c_int, [_c_vp, _c_i64, _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_f, _c_int, _c_i64,
                                        _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                        _c_vp, _c_i64, _c_int, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp, _c_i64, _c_vp,
                                        _c_i64, _c_vp, _c_i64, _c_vp, _c_int, _c_vp, _c_int, _c_vp]),
    "trlx_ppo_sample_proc": (_c_int, [ctypes.POINTER(PpoSampleProcArgs), _c_vp]),
    "trlx_ppo_sample_proc_dev": (_c_int, [ctypes.POINTER(PpoSampleProcArgs), ctypes.POINTER(PpoSampleDevArgs),
                                          _c_vp]),
    "trlx_t5_decode_attn": (_c_int, [ctypes.POINTER(T5DecodeAttnArgs), _c_vp]),
    "trlx_decode_clock_init": (_c_int, [_c_vp, _c_i64, _c_i64, _c_vp]),
    "trlx_decode_clock_advance": (_c_int, [_c_vp, _c_vp]),
    "trlx_t5_decode_attn_dev": (_c_int, [ctypes.POINTER(T5DecodeAttnArgs), _c_vp, _c_vp]),
    "trlx_t5_decode_attn_live": (_c_int, [ctypes.POINTER(T5DecodeAttnArgs), _c_vp, _c_vp, _c_vp]),
    "trlx_t5_cross_kv_quantize": (_c_int, [ctypes.POINTER(T5CrossKvQuantArgs), _c_vp]),
    "trlx_t5_decode_attn_kv8": (_c_int, [ctypes.POINTER(T5DecodeAttnArgs), _c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_t5_decode_attn_group": (_c_int, [ctypes.POINTER(T5DecodeAttnGroupArgs), _c_vp]),
    "trlx_t5_decode_attn_group_tile": (_c_int, [_c_i64]),
    "trlx_t5_decode_attn_split": (_c_int, [ctypes.POINTER(T5DecodeAttnGroupArgs), _c_i64, _c_vp, _c_i64, _c_vp]),
    "trlx_t5_decode_attn_split_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    "trlx_t5_decode_attn_split_geometry": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64,
                                                    ctypes.POINTER(T5DecodeAttnSplitGeometry)]),
    "trlx_t5_decode_attn_split_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64]),
    "trlx_t5_decode_embed": (_c_int, [ctypes.POINTER(T5DecodeEmbedArgs), _c_vp, _c_vp]),
    "trlx_t5_attention": (_c_int, [ctypes.POINTER(T5AttentionArgs), _c_vp]),
    "trlx_t5_attention_tiles": (_c_int, [ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "trlx_t5_attention_fwd_lse": (_c_int, [ctypes.POINTER(T5AttentionArgs), _c_vp, _c_vp]),
    "trlx_t5_attention_bwd": (_c_int, [ctypes.POINTER(T5AttentionBwdArgs), _c_vp]),
    "trlx_t5_attention_bwd_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "trlx_t5_attention_bwd_tiles": (_c_int, [ctypes.POINTER(_c_int)] * 4),
    "trlx_t5_ff_act_fwd": (_c_int, [ctypes.POINTER(T5FfActArgs), _c_vp]),
    "trlx_t5_ff_act_bwd": (_c_int, [ctypes.POINTER(T5FfActArgs), _c_vp]),
    "trlx_t5_ff_act_geometry": (_c_int, [ctypes.POINTER(_c_int)] * 4),
    "trlx_t5_rmsnorm_fwd": (_c_int, [ctypes.POINTER(T5RmsNormArgs), _c_vp]),
    "trlx_t5_rmsnorm_bwd": (_c_int, [ctypes.POINTER(T5RmsNormArgs), _c_vp]),
    "trlx_t5_rmsnorm_geometry": (_c_int, [_c_i64, _c_i64, ctypes.POINTER(T5RmsNormGeometry)]),
    "trlx_t5_decode_linear": (_c_int, [ctypes.POINTER(T5DecodeLinearArgs), _c_vp]),
    "trlx_t5_decode_linear_geometry": (_c_int, [ctypes.POINTER(T5DecodeLinearGeometry)]),
    "trlx_t5_decode_linear_rows": (_c_int, [ctypes.POINTER(T5DecodeLinearRowsArgs), _c_vp]),
    "trlx_t5_decode_linear_rows_geometry": (_c_int, [ctypes.POINTER(T5DecodeLinearRowsGeometry)]),
    "trlx_rows_copy": (_c_int, [_c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp,
                                _c_i64, _c_vp, _c_i64, _c_vp]),
    "trlx_shift_tokens_right": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp]),
    "trlx_ilql_collate": (_c_int, [_c_vp] * 9 + [_c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64]
                          + [_c_vp, _c_i64] * 6 + [_c_vp]),
    "trlx_ilql_build_fields": (_c_int, [_c_vp] * 6 + [_c_i64] * 4 + [_c_vp] * 6),
    "trlx_ctl_init": (_c_int, [_c_vp, _c_d, _c_d, _c_d, _c_int, _c_vp]),
    "trlx_score_moments": (_c_int, [_c_vp, _c_int, _c_i64, _c_vp, _c_vp]),
    "trlx_score_moments_signal": (_c_int, [_c_vp, _c_int, _c_i64, _c_vp, _c_vp, _c_vp]),
    "trlx_score_ctl_update": (_c_int, [_c_vp, _c_int, _c_i64, _score_ctl_p, _c_vp, _c_int, _c_vp]),
    "trlx_kl_ctl_update": (_c_int, [_kl_ctl_p, _c_vp, _c_vp]),
    "trlx_ppo_rollout_gae_ctl": (_c_int, [_c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp,
                                          _score_ctl_p, _c_d, _c_d, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp,
                                          _c_vp]),
    "trlx_ppo_rollout_loss_ctl": (_c_int, [_c_i64, _c_i64, _c_vp, _c_f, _c_vp, _c_vp, _c_vp, _kl_ctl_p, _c_vp]),
    "trlx_ppo_rollout_gae_split": (_c_int, [_c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp,
                                            _score_ctl_p, _c_f, _c_d, _c_d, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                            _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "trlx_score_moments_merge": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp]),
    "trlx_ppo_whiten_coef": (_c_int, [_c_vp, _c_int, _c_vp, _c_f, _c_vp, _c_vp]),
    "trlx_ppo_loss_rows_split": (_c_int, [_c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                          _c_i64, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                          _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_int, _c_f, _c_f, _c_f,
                                          _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "trlx_ppo_loss_rows_split_gae": (_c_int, [_c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64,
                                              _c_i64, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp,
                                              _c_f, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_vp,
                                              _c_int, _c_f, _c_f, _c_f, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp,
                                              _gae_split_p, _c_vp, _c_vp]),
    "trlx_comm_load": (_c_int, [ctypes.c_char_p]),
    "trlx_comm_unique_id_bytes": (_c_i64, []),
    "trlx_comm_unique_id": (_c_int, [_c_vp, _c_i64]),
    "trlx_comm_init": (_c_int, [ctypes.POINTER(ctypes.c_void_p), _c_vp, _c_i64, _c_int, _c_int]),
    "trlx_comm_allreduce_sum_f64": (_c_int, [_c_vp, _c_vp, _c_i64, _c_vp]),
    "trlx_comm_destroy": (_c_int, [_c_vp]),
    "trlx_lsm_gather_fwd_loss_tail": (_c_int, [_c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp,
                                               _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_i64, _c_i64,
                                               _c_vp, _c_f, _c_vp, _c_vp, _c_vp, _kl_ctl_p, _c_vp]),
    "trlx_ilql_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64, _c_int]),
    "trlx_ilql_prep": (_c_int, [_ilql_p, _c_vp]),
    "trlx_ilql_rows": (_c_int, [_ilql_p, _c_vp]),
    "trlx_ilql_finalize": (_c_int, [_ilql_p, _c_vp]),
    "trlx_ilql_loss_fused": (_c_int, [_ilql_p, _c_vp]),
    "trlx_ilql_tq_at_actions": (_c_int, [_ilql_tq_p, _c_vp]),
    "trlx_polyak_update": (_c_int, [ctypes.POINTER(_c_vp), ctypes.POINTER(_c_vp), ctypes.POINTER(_c_i64), _c_i64,
                                    _c_int, _c_d, _c_vp]),
    "trlx_adamw_step": (_c_int, [_adamw_p, _c_vp]),
    "trlx_grad_norm_workspace_bytes": (_c_i64, [ctypes.POINTER(_c_i64), _c_i64]),
    "trlx_grad_norm": (_c_int, [_grad_norm_p, _c_vp]),
    "trlx_adamw_step_clipped": (_c_int, [_adamw_p, _c_vp, _c_vp]),
    "trlx_adamw_advance": (_c_int, [ctypes.POINTER(AdamwAdvanceArgs), _c_vp]),
    "trlx_adamw_sched_scalars_host": (_c_int, [_c_i64, _c_d, _c_d, _c_d, _c_d, _c_d, _c_d,
                                               ctypes.POINTER(_c_f)]),
    "trlx_adamw_step_dev": (_c_int, [_adamw_p, _c_vp, _c_vp]),
    "trlx_adamw_step_clipped_dev": (_c_int, [_adamw_p, _c_vp, _c_vp, _c_vp]),
    "trlx_adamw_step_ex": (_c_int, [_adamw_p, _c_int, _c_vp, _c_vp, _c_vp]),
    "trlx_value_head_splits": (_c_int, [_c_i64, _c_i64]),
    "trlx_value_head_workspace_bytes": (_c_i64, [_c_i64, _c_i64]),
    "trlx_value_head_bwd_workspace_bytes": (_c_i64, [_c_i64, _c_i64]),
    "trlx_value_head_fwd": (_c_int, [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_int,
                                     _c_vp, _c_vp]),
    "trlx_value_head_bwd": (_c_int, [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_i64, _c_i64, _c_vp,
                                     _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp]),
}

_lib = None


class TrlxError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle; raises if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TrlxError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `python -c 'import "
            f"__graft_entry__ as g; g.build()'` or `make -C trlx-t5_amd/csrc`). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.trlx_abi_version() != ABI_VERSION:
        raise TrlxError(f"ABI mismatch: library {lib.trlx_abi_version()} vs binding {ABI_VERSION}")
    _lib = lib
    return lib


def call(name, *args):
    """Invoke a status-returning entry point; raise on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.trlx_last_error().decode(errors="replace")
        err = ValueError if rc in (1, 2, 3, 5) else TrlxError
        raise err(f"{name} failed (status {rc}): {msg}")
    return rc


_TUNED = {}  # the values set through this binding (the library keeps no getter); unset = 0 (auto)


def set_tuning(key: str, value: int):
    """Launch-geometry knob (see trlx_set_tuning in include/trlx_t5_amd.h).  The knobs are
    process-wide (common.h TuneKnob): a value set here reaches every host thread's launches,
    autograd's backward thread included."""
    call("trlx_set_tuning", key.encode(), int(value))
    _TUNED[key] = int(value)


@contextlib.contextmanager
def tuning(**knobs):
    """Set knobs for the duration of a block and restore the values they had before (the ones
    set through set_tuning, else 0 = auto), also when the block raises."""
    prev = {k: _TUNED.get(k, 0) for k in knobs}
    try:
        for k, v in knobs.items():
            set_tuning(k, v)
        yield
    finally:
        for k, v in prev.items():
            set_tuning(k, v)


def query(name, *args):
    return getattr(load(), name)(*args)


# ------------------------------------------------------------------ tensor helpers
def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.int64:
        return I64
    raise TypeError(f"unsupported dtype {t.dtype} (trlx_t5_amd kernels take float32 / bfloat16 / int64)")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream_of(t):
    """hipStream_t (as int) of torch's current stream on t's device."""
    return torch.cuda.current_stream(t.device).cuda_stream


def require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("trlx_t5_amd: tensors must live on a ROCm (cuda) device; there is no CPU path")
