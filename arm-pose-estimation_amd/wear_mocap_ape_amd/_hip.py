"""ctypes binding of libape_hip.so (C ABI: include/ape_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``csrc/Makefile`` into
``arm-pose-estimation_amd/lib/``.  Loading failures are loud: there is no CPU fallback."""
import ctypes as C
import os
from pathlib import Path

# torch FIRST: it loads the HIP runtime (libamdhip64.so.7) that owns the device pointers and streams
# handed to the kernels; libape_hip.so must bind to that same loaded runtime, not open a second copy.
import torch  # noqa: F401

LIB_PATH = Path(os.environ.get("APE_HIP_LIB", Path(__file__).resolve().parents[1] / "lib" / "libape_hip.so"))

APE_OK = 0
LAYOUT_NONE = -1
LAYOUT_ORI_CAL_LARM_UARM_HIPS = 0
LAYOUT_ORI_CAL_LARM_UARM = 1
LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS = 2
F32, F64 = 0, 1
FLAG_NORMALIZE_INPUT = 0x1
FLAG_ALL_STEPS = 0x2
FLAG_DROPOUT_MASKS = 0x4
FLAG_DROPOUT_PHILOX = 0x8
FLAG_PACKED_MSG = 0x20
FLAG_BROADCAST_X = 0x10
FLAG_SPREAD = 0x40                # frames, banks, replays: every output row ends in the spread record
SPREAD_WIDTH = 21                 # APE_SPREAD_WIDTH
SCORE_WIDTH, SCORE_ACC_WIDTH = 7, 25        # APE_SCORE_WIDTH, APE_SCORE_ACC_WIDTH (ape_score_rows)
TRUTH_TARGETS, TRUTH_EST = 0, 1             # APE_TRUTH_*
SCORE_MAX_LAG, SCORE_MAX_LAGS = 128, 65      # APE_SCORE_MAX_LAG, APE_SCORE_MAX_LAGS (ape_score_lags)
POST_MAX_CONFIGS = 64             # APE_POST_MAX_CONFIGS (ape_post_sweep)
POST_MAX_WINDOW = 64              # APE_POST_MAX_WINDOW (ape_post_window)
SELECT_MAX_EDGES, SELECT_MAX_SLOPE = 256, 8    # APE_SELECT_MAX_EDGES, APE_SELECT_MAX_SLOPE (ape_select_rungs)
SEGMENT_MAX_MIN, SEG_TABLE_WIDTH, SEG_MAX_VALUES, SEG_STAT_WIDTH, SEG_PIECE = 256, 4, 16, 5, 1024    # APE_SEGMENT_MAX_MIN, APE_SEG_* (ape_segment_*)
FRAME_ACC_WIDTH = 51              # APE_FRAME_ACC_WIDTH (ape_frame_sums)
BODY_ACC_WIDTH = 46               # APE_BODY_ACC_WIDTH (ape_body_sums)
BODY_ROT_MSG, BODY_ROT_TRUTH = 0, 1         # APE_BODY_ROT_*
MOTION_WIDTH, MOTION_ACC_WIDTH = 12, 38     # APE_MOTION_WIDTH, APE_MOTION_ACC_WIDTH (ape_motion_sums)
ROWS_MSG, ROWS_EST, ROWS_TARGETS = 0, 1, 2  # APE_ROWS_*
HIST_MAX_BINS, HIST_MAX_WIDTH = 256, 16     # APE_HIST_MAX_BINS, APE_HIST_MAX_WIDTH (ape_score_hist)
ANGLE_WIDTH, ANGLE_ACC_WIDTH = 7, 71        # APE_ANGLE_WIDTH, APE_ANGLE_ACC_WIDTH (ape_joint_angles)
BY_MAX_KEYS, BY_MAX_VALUES, BY_MAX_BINS, BY_PIECE = 8, 16, 125, 1024    # APE_BY_* (ape_score_by)
SPECTRA_DETREND, SPECTRA_MAX_N, SPECTRA_MAX_COLS = 0x1, 512, 16        # APE_SPECTRA_* (ape_spectra)
FIT_PIECE, FIT_MAX_P, FIT_MAX_Q = 512, 256, 32        # APE_FIT_* (ape_fit_sums)
FLAG_ANY_PLACEMENT, FLAG_NO_XCD_CLASSES, FLAG_ALT_FORM = 0x08000000, 0x02000000, 0x01000000    # exchange-form selectors (A/B runs, tests)
FLAG_IN_XCD_PLAIN = 0x00400000      # opt-in: plain hand-over stores inside an XCD-pure cluster (the default is write-through)
KERNEL_AUTO, KERNEL_TILE16, KERNEL_CLUSTER, KERNEL_CLUSTER_GEN1, KERNEL_AUTO_GEN1 = 0, 1, 2, 3, 4
PRECISION_F32, PRECISION_F16, PRECISION_F16_GEN1 = 0, 1, 2
MODEL_LSTM, MODEL_FF, MODEL_IMUPOSE = 0, 1, 2
PARSE_WATCH_PHONE_POCKET, PARSE_WATCH_ONLY, PARSE_WATCH_ONLY_PHONE_MSG, PARSE_WATCH_PHONE_UARM = 0, 1, 2, 3
PARSE_SHAPES = {0: (55, 22), 1: (28, 20), 2: (55, 20), 3: (55, 38)}
PARSE_BIG_ENDIAN = 0x100          # OR-ed into a kind: rows are big-endian float32 (the UDP payload as received)
ABI_VERSION = 7

EST_WIDTH = {LAYOUT_ORI_CAL_LARM_UARM_HIPS: 21, LAYOUT_ORI_CAL_LARM_UARM: 14, LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS: 21}
NUM_TARGETS = {LAYOUT_ORI_CAL_LARM_UARM_HIPS: 14, LAYOUT_ORI_CAL_LARM_UARM: 12, LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS: 20}


class ApeDims(C.Structure):
    _fields_ = [("input_size", C.c_int32), ("hidden_size", C.c_int32), ("num_layers", C.c_int32),
                ("output_size", C.c_int32), ("target_layout", C.c_int32), ("device", C.c_int32),
                ("model_kind", C.c_int32)]


class ApeModelStats(C.Structure):
    _fields_ = [("aborted_checks", C.c_uint64), ("reissued_calls", C.c_uint64), ("lost_calls", C.c_uint64)]


class ApeKalmanDims(C.Structure):
    _fields_ = [("num_ensemble", C.c_int32), ("win_size", C.c_int32), ("device", C.c_int32)]


STATE_VERSION, STATE_WINDOW_WARM, STATE_STACK_WARM = 1, 1, 2


class ApeStreamStateDesc(C.Structure):
    """``ape_stream_state_desc_t``: the shape of a bank's canonical per-stream record"""
    _fields_ = [("version", C.c_int32), ("T", C.c_int32), ("I", C.c_int32), ("smooth", C.c_int32), ("n_mc", C.c_int32),
                ("O", C.c_int32), ("words_per_stream", C.c_int32)]


KALMAN_STATE_VERSION = 1


class ApeKalmanStateDesc(C.Structure):
    """``ape_kalman_state_desc_t``: the shape of a Kalman bank's canonical per-stream record"""
    _fields_ = [("version", C.c_int32), ("E", C.c_int32), ("W", C.c_int32), ("smooth", C.c_int32), ("words_per_stream", C.c_int32)]


# every symbol include/ape_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "ape_abi_version": (C.c_int, []),
    "ape_last_error": (C.c_char_p, []),
    "ape_device_count": (C.c_int, []),
    "ape_model_create": (C.c_int, [C.POINTER(ApeDims), C.POINTER(C.c_void_p)]),
    "ape_model_destroy": (C.c_int, [C.c_void_p]),
    "ape_model_reserve": (C.c_int, [C.c_void_p, C.c_int32]),
    "ape_model_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ape_weight_blob_floats": (C.c_size_t, [C.POINTER(ApeDims)]),
    "ape_model_set_norm_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_double)] * 4),
    "ape_model_set_body": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ape_lstm_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p,
                                   C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]),
    "ape_lstm_forward_hs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p,
                                      C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ape_fk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ape_msg_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_streams_last_post_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "ape_spread_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ape_parse_rows": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ape_streams_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "ape_streams_destroy": (C.c_int, [C.c_void_p]),
    "ape_streams_reset": (C.c_int, [C.c_void_p]),
    "ape_streams_set_mc": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_uint64]),
    "ape_streams_push_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_streams_push_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ape_streams_step": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ape_streams_frame_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ape_streams_frame_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "ape_infer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_int32, C.c_void_p]),
    "ape_replay": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                             C.c_int32, C.c_float, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                             C.c_void_p]),
    "ape_streams_reset_subset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "ape_streams_frame_subset": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p,
                                           C.c_int32, C.c_void_p]),
    "ape_fk_bank_create": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_void_p)]),
    "ape_fk_bank_destroy": (C.c_int, [C.c_void_p]),
    "ape_fk_bank_reset": (C.c_int, [C.c_void_p]),
    "ape_fk_bank_reset_subset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "ape_fk_bank_frame": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ape_fk_bank_frame_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ape_fk_replay": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    # per-stream body measurements: bank, stream list, K, [K,9] float64 values, HIP stream / bank, [S,9] out
    "ape_streams_set_bodies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_streams_get_bodies": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ape_fk_bank_set_bodies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_fk_bank_get_bodies": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ape_kalman_bank_set_bodies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_kalman_bank_get_bodies": (C.c_int, [C.c_void_p, C.c_void_p]),
    # per-stream smoothing lengths: bank, stream list, K, [K] int32 values, HIP stream / bank, [S] int32 out
    "ape_streams_set_smooths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_streams_get_smooths": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ape_fk_bank_set_smooths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_fk_bank_get_smooths": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ape_model_set_kernel": (C.c_int, [C.c_void_p, C.c_int32]),
    "ape_model_set_precision": (C.c_int, [C.c_void_p, C.c_int32]),
    "ape_model_check": (C.c_int, [C.c_void_p]),
    "ape_model_recover": (C.c_int, [C.c_void_p]),
    "ape_model_stats": (C.c_int, [C.c_void_p, C.POINTER(ApeModelStats)]),
    "ape_streams_profile": (C.c_int, [C.c_void_p, C.c_int32]),
    "ape_streams_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "ape_lstm_kernel_name": (C.c_char_p, [C.c_void_p, C.c_int32, C.c_int32]),
    "ape_model_last_kernel": (C.c_char_p, [C.c_void_p]),
    "ape_flops_per_window": (C.c_double, [C.POINTER(ApeDims), C.c_int32]),
    "ape_kalman_create": (C.c_int, [C.POINTER(ApeKalmanDims), C.POINTER(C.c_void_p)]),
    "ape_kalman_destroy": (C.c_int, [C.c_void_p]),
    "ape_kalman_weight_floats": (C.c_size_t, [C.c_void_p]),
    "ape_kalman_noise_floats": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "ape_kalman_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ape_kalman_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p] + [C.c_void_p] * 6),
    "ape_kalman_format_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ape_kalman_check": (C.c_int, [C.c_void_p]),
    "ape_kalman_bank_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "ape_kalman_bank_destroy": (C.c_int, [C.c_void_p]),
    "ape_kalman_bank_reset": (C.c_int, [C.c_void_p]),
    "ape_kalman_bank_reset_subset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "ape_kalman_bank_set_norm_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_double)] * 4),
    "ape_kalman_bank_set_body": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "ape_kalman_bank_set_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ape_kalman_bank_frame": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ape_kalman_bank_frame_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ape_kalman_replay": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] +
                          [C.POINTER(C.c_double)] * 5 + [C.c_uint64, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# the replays with one body per recording: every argument of the plain entry, then bodies_host [R,9] float64 (or NULL)
for _name in ("ape_replay", "ape_fk_replay", "ape_kalman_replay"):
    SIGNATURES[_name + "_bodies"] = (C.c_int, SIGNATURES[_name][1] + [C.c_void_p])
# ape_replay_bodies for every regressor kind the loader dispatches (DropoutFF, ImuPoseLSTM)
SIGNATURES["ape_replay_regressor"] = SIGNATURES["ape_replay_bodies"]
SIGNATURES["ape_replay_resume"] = (C.c_int, SIGNATURES["ape_replay_bodies"][1] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64])
# stream state hand-over: the same trio on the regressor banks and the FK-only bank
for _bank in ("ape_streams", "ape_fk_bank"):
    SIGNATURES[_bank + "_state_desc"] = (C.c_int, [C.c_void_p, C.POINTER(ApeStreamStateDesc)])
    SIGNATURES[_bank + "_export"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
    SIGNATURES[_bank + "_import"] = (C.c_int, [C.c_void_p, C.POINTER(ApeStreamStateDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p])
# the Kalman bank's state hand-over: records with int32 ages, the bank's draw position, the resumable replay
SIGNATURES["ape_kalman_bank_state_desc"] = (C.c_int, [C.c_void_p, C.POINTER(ApeKalmanStateDesc)])
SIGNATURES["ape_kalman_bank_export"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
SIGNATURES["ape_kalman_bank_import"] = (C.c_int, [C.c_void_p, C.POINTER(ApeKalmanStateDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p])
SIGNATURES["ape_kalman_bank_get_draw_position"] = (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
SIGNATURES["ape_kalman_bank_set_draw_position"] = (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64])
SIGNATURES["ape_kalman_replay_resume"] = (C.c_int, SIGNATURES["ape_kalman_replay_bodies"][1] +
                                          [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64])
# host subset frames: bank, kind, rows_host, streams_host, K, [flags,] out_host, out_dtype, [n_rows_host,] HIP stream
SIGNATURES["ape_streams_frame_subset_host"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p,
                                                         C.c_int32, C.c_void_p])
SIGNATURES["ape_fk_bank_frame_subset_host"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                         C.c_void_p])
SIGNATURES["ape_kalman_bank_frame_subset_host"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p,
                                                             C.c_int32, C.c_void_p, C.c_void_p])
# scoring against ground truth: layout, msg + stride, spread + stride, msg dtype, truth + kind + dtype, F, starts_host, R,
# skip, bodies_host, n_bodies, score + dtype, acc, HIP stream
SIGNATURES["ape_score_rows"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p])
# the same over a sweep of lags: ... n_bodies, lag_min, lag_max, rec_lag_host, score + dtype, acc, HIP stream
SIGNATURES["ape_score_lags"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
# post-filter sweep: model, y, F, n_mc, starts_host, R, configs_host [C,2], C, flags, bodies_host, n_bodies, out + dtype,
# workspace_bytes, HIP stream; and the debug counter of the last call's plan (passes, frames per pass, frames per tile, staged in LDS)
SIGNATURES["ape_post_sweep"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p])
SIGNATURES["ape_post_sweep_last"] = (C.c_int, [C.POINTER(C.c_int32)])
# windowed post-filter: model, y, F, n_mc, starts_host, R, windows_host [C,3], weights_host [C,64] or NULL, C, flags,
# bodies_host, n_bodies, out + dtype, workspace_bytes, HIP stream; and the debug counter of the last call's plan
SIGNATURES["ape_post_window"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p])
SIGNATURES["ape_post_window_last"] = (C.c_int, [C.POINTER(C.c_int32)])
# a window per frame from a ladder.  The post-filter: ape_post_window's arguments with sel [S, F] (device) and S behind the
# ladder's L; and the debug counter of the last call's plan.  The selector: keys + dtype, n_sets, set_stride (int64), F, frame_stride
# (int64), starts_host, R, edges_host [B], B, rung_of_slot_host [B + 1], nan_rung, reach_host [L], L, slope, sel, HIP stream
SIGNATURES["ape_post_select"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p])
SIGNATURES["ape_post_select_last"] = (C.c_int, [C.POINTER(C.c_int32)])
SIGNATURES["ape_select_rungs"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p])
# reaches and holds.  The labeller: keys + dtype, S, set stride, F, frame stride, starts_host, R, thresholds_host [P, 2],
# mins_host [P, 2], P, first_label, labels, HIP stream.  The table: labels, S, F, starts_host, R, seg_of_frame | NULL, n_segs, table, cap,
# HIP stream.  The reductions: values + dtype, value sets, set / frame / column stride, V, S, F, seg_of_frame, table, n_segs, cap, out,
# HIP stream.
SIGNATURES["ape_segment_frames"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p])
SIGNATURES["ape_segment_runs"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_void_p])
SIGNATURES["ape_segment_stats"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
# heading and frame offset against the truth.  The sums: layout, msg + stride, msg dtype, truth + kind + dtype, F,
# starts_host, R, skip, bodies_host, n_bodies, lag_min, lag_max, rec_lag_host, acc, HIP stream.  The rotation: layout, msg + stride,
# spread + stride, msg dtype, F, starts_host, R, quats_host, n_quats, out + dtype, HIP stream
SIGNATURES["ape_frame_sums"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
SIGNATURES["ape_rotate_rows"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p])
# mocap truth on each frame's clock.  The clock: dt + stride + dtype, flags, F, starts_host, R, times, HIP stream.  The
# rows: layout, truth + kind + dtype, Ft, truth_starts_host, truth_times, times, F, starts_host, R, shift_host, max_gap, bodies_host,
# n_bodies, out + dtype, HIP stream
SIGNATURES["ape_frame_times"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
SIGNATURES["ape_resample_truth"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                              C.c_void_p])
# arm lengths and shoulder origin against the truth.  The sums: layout, msg + stride, msg dtype, truth + kind + dtype, F,
# starts_host, R, skip, rot_source, lag_min, lag_max, rec_lag_host, acc, HIP stream.  The rows: layout, msg + stride, msg dtype, F,
# starts_host, R, bodies_host, n_bodies, out + dtype, HIP stream
SIGNATURES["ape_body_sums"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
SIGNATURES["ape_rebody_rows"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_void_p])
# speed, acceleration and jerk of every frame: layout, rows + kind + stride + dtype, n_sets, set_stride (int64), F,
# starts_host, R, skip, times, bodies_host, n_bodies, motion + dtype, acc, HIP stream
SIGNATURES["ape_motion_sums"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p])
# counts of per-frame values over fixed edges: values + dtype, width, n_sets, set_stride (int64), F, frame_stride (int64),
# n_groups, group_stride (int64), starts_host, R, trim_host, edges_host, n_bins, hist, HIP stream
SIGNATURES["ape_score_hist"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
# joint angles of every frame and their errors against truth: layout, rows + kind + stride + dtype, n_sets, set_stride
# (int64), truth + kind + stride + dtype, rec_lag_host, F, starts_host, R, skip, bodies_host, n_bodies, min_swing, angles, errors, out dtype,
# acc, HIP stream
SIGNATURES["ape_joint_angles"] = (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                            C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
# per-slot sums of value columns keyed by other columns: keys + dtype, n_keys, set and frame stride (int64), values + dtype,
# n_values, set and frame stride (int64), n_sets, F, starts_host, R, trim_host, edges_host, n_bins, by, HIP stream
SIGNATURES["ape_score_by"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                        C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p])
# Welch sums per frequency: x + dtype, set and frame stride (int64), x_cols_host, y | NULL + dtype, set and frame stride
# (int64), y_cols_host, V, n_sets, F, starts_host, R, skip, N, hop, taper_host, flags, acc, counts, HIP stream
SIGNATURES["ape_spectra"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
# the output layer fitted to a wearer.  Features: ape_lstm_forward's arguments with h in front of y.  Replay features:
# model, kind, rows, F, starts_host, R, seq_len, flags, h, y | NULL, max_rows_per_launch, HIP stream.  The sums: x + stride (int64) + dtype,
# P, t + stride (int64) + dtype, Q, shift_host | NULL, scale_host | NULL, F, starts_host, R, skip, rec_lag_host | NULL, acc, HIP stream.
# The head: model, w_out_host [O, H] float32, b_out_host [O] float32
SIGNATURES["ape_lstm_features"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_float, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.c_void_p])
SIGNATURES["ape_replay_features"] = (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
SIGNATURES["ape_fit_sums"] = (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
SIGNATURES["ape_model_set_head"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
SIGNATURES["ape_model_get_head"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])

_lib = None


def lib():
    """The loaded library; raises ``UserWarning`` (the reference's error convention) if the HIP
    extension has not been built -- the product path never degrades to a CPU implementation."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise UserWarning(f"HIP extension missing: {LIB_PATH} (run `python -c 'import __graft_entry__ as g; "
                              f"g.build()'` or `make -C arm-pose-estimation_amd/csrc`)")
        handle = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.ape_abi_version() != ABI_VERSION:
            raise UserWarning(f"{LIB_PATH}: ABI version {handle.ape_abi_version()} != {ABI_VERSION}")
        _lib = handle
    return _lib


def check(status: int, what: str = ""):
    """non-zero status -> ``UserWarning`` raised as an exception (nn_models.py:385-400 convention)."""
    if status != APE_OK:
        msg = lib().ape_last_error().decode("utf-8", "replace")
        raise UserWarning(f"[ape_hip] {what}: {msg} (status {status})")


def dptr(array_like, dtype):
    return array_like.ctypes.data_as(C.POINTER(dtype))
