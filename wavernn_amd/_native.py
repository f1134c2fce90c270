"""ctypes binding of the C-ABI (include/wavernn_amd.h) in libwavernn_amd.so.

The product path has no fallback: if the HIP library is missing or cannot be loaded this
module raises, it never substitutes a CPU implementation."""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_lib", "libwavernn_amd.so")

ABI_VERSION = 7
MODE_RAW, MODE_MOL, MODE_DM = 0, 1, 2
STATUS = {0: "WRNN_OK", -1: "WRNN_EINVAL", -2: "WRNN_EHIP", -3: "WRNN_ENOWEIGHTS", -4: "WRNN_ETIMEOUT",
          -5: "WRNN_ENOMEM", -6: "WRNN_EUNSUPPORTED"}

# Every symbol include/wavernn_amd.h declares (tests check the .so exports all of them).
EXPORTS = ("wrnn_create", "wrnn_set_weights", "wrnn_generate", "wrnn_check", "wrnn_elapsed_ms",
           "wrnn_query", "wrnn_last_error", "wrnn_destroy", "wrnn_cond_shape", "wrnn_upsample_pack",
           "wrnn_postprocess", "wrnn_cond_last_error", "wrnn_generate_frames", "wrnn_generate_frames_rows",
           "wrnn_frame_weights", "wrnn_melresnet_floats", "wrnn_melresnet", "wrnn_philox_draws",
           "wrnn_melresnet_tile_frames", "wrnn_stream_open", "wrnn_stream_push", "wrnn_stream_plan",
           "wrnn_stream_lookahead", "wrnn_stream_close", "wrnn_stream_push_group", "wrnn_fingerprint",
           "wrnn_list_plan", "wrnn_generate_list", "wrnn_stream_open_wide", "wrnn_wide_plan",
           "wrnn_stream_mu_law", "wrnn_wide_steps_per_launch", "wrnn_list_wide_plan", "wrnn_generate_list_wide",
           "wrnn_postprocess_list", "wrnn_list_folds_plan", "wrnn_generate_list_folds", "wrnn_postprocess_list_folds",
           "wrnn_stream_open_rows", "wrnn_upsample_pack_window", "wrnn_upsample_window_frames",
           "wrnn_melspec_frames", "wrnn_melspec_table_floats", "wrnn_melspec_tables", "wrnn_melspec",
           "wrnn_melspec_window", "wrnn_melspec_windows", "wrnn_melspec_plan", "wrnn_taco_supported",
           "wrnn_taco_state_floats", "wrnn_taco_state_layout", "wrnn_taco_scratch_floats", "wrnn_taco_run",
           "wrnn_cbhg_supported", "wrnn_cbhg_scratch_bytes", "wrnn_cbhg_scratch_layout", "wrnn_cbhg_run")
MELSPEC_SCRATCH_PER_SIGNAL = 64


class MelResNetCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("in_dims", "compute_dims", "res_out_dims", "res_blocks", "pad")]


class MelSpecCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("sample_rate", "n_fft", "hop_length", "win_length", "num_mels")] + \
        [("fmin", ctypes.c_float), ("min_level_db", ctypes.c_float)]


TACO_WEIGHTS = ("prenet_fc1_w", "prenet_fc1_b", "prenet_fc2_w", "prenet_fc2_b", "attn_rnn_w_ih", "attn_rnn_w_hh",
                "attn_rnn_b_ih", "attn_rnn_b_hh", "lsa_conv_w", "lsa_L_w", "lsa_L_b", "lsa_W_w", "lsa_W_b", "lsa_v",
                "rnn_input_w", "rnn_input_b", "res_rnn1_w_ih", "res_rnn1_w_hh", "res_rnn1_b_ih", "res_rnn1_b_hh",
                "res_rnn2_w_ih", "res_rnn2_w_hh", "res_rnn2_b_ih", "res_rnn2_b_hh", "mel_proj_w")
TACO_STATE_FIELDS = ("attn_hidden", "rnn1_hidden", "rnn1_cell", "rnn2_hidden", "rnn2_cell", "context", "cumulative",
                     "attention", "frame", "step", "stopped")


class TacoCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_mels", "decoder_dims", "lstm_dims", "encoder_dims", "prenet_fc1",
                                              "prenet_fc2", "lsa_filters", "lsa_kernel", "max_r")]


class TacoWeights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in TACO_WEIGHTS]


CBHG_MAX_K, CBHG_HIGHWAYS = 16, 4
CBHG_STAGES = ("front", "bank", "pooled", "proj1", "residual", "highway_in", "highway_out", "gi", "rnn")


class CbhgCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("K", "in_channels", "channels", "proj1", "proj2", "pre_highway", "highways",
                                              "front", "embed_dims", "num_chars", "prenet_fc1", "tail_out")]


class CbhgWeights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("embedding", "prenet_fc1_w", "prenet_fc1_b", "prenet_fc2_w", "prenet_fc2_b")] + \
        [(n, ctypes.c_void_p * CBHG_MAX_K) for n in ("bank_w", "bank_bn_w", "bank_bn_b", "bank_bn_mean", "bank_bn_var")] + \
        [(n, ctypes.c_void_p) for n in ("proj1_w", "proj1_bn_w", "proj1_bn_b", "proj1_bn_mean", "proj1_bn_var",
                                        "proj2_w", "proj2_bn_w", "proj2_bn_b", "proj2_bn_mean", "proj2_bn_var")] + \
        [("pre_highway_w", ctypes.c_void_p)] + \
        [(n, ctypes.c_void_p * CBHG_HIGHWAYS) for n in ("hw_w1", "hw_b1", "hw_w2", "hw_b2")] + \
        [(n, ctypes.c_void_p) for n in ("rnn_w_ih", "rnn_w_hh", "rnn_b_ih", "rnn_b_hh", "rnn_w_ih_r", "rnn_w_hh_r",
                                        "rnn_b_ih_r", "rnn_b_hh_r", "tail_w")]


class WrnnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class WrnnInvalid(WrnnError, ValueError):
    """WRNN_EINVAL: an argument the library refused before it queued anything (also a ValueError)."""


class Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("abi_version", "mode", "rnn_dims", "fc_dims", "aux_dims",
                                              "feat_dims", "n_classes", "grid", "timeout_ms")]


class Tensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("numel", ctypes.c_int64),
                ("on_device", ctypes.c_int32)]


class Info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("grid", "units_rnn", "units_fc", "units_cls", "max_rows",
                                              "lds_bytes", "slab_floats", "num_cus", "rows_grid",
                                              "rows_units_rnn", "sparse_blocks", "split_grid", "last_path",
                                              "xcd_rows", "xcdm_rows", "last_row_groups", "last_row_blocks",
                                              "last_block_rows", "last_tile_rows")]


class UpsampleCfg(ctypes.Structure):
    _fields_ = [("feat_dims", ctypes.c_int32), ("res_out_dims", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("n_scales", ctypes.c_int32), ("scales", ctypes.c_int32 * 4),
                ("taps", ctypes.POINTER(ctypes.c_float) * 4)]


_lib = None


def lib() -> ctypes.CDLL:
    """Load libwavernn_amd.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extension with "
                          "`python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    L.wrnn_create.argtypes = [ctypes.POINTER(Config), i32, ctypes.POINTER(vp)]
    L.wrnn_create.restype = i32
    L.wrnn_set_weights.argtypes = [vp, ctypes.POINTER(Tensor), i32]
    L.wrnn_set_weights.restype = i32
    L.wrnn_generate.argtypes = [vp, vp, i32, i32, vp, u64, i64, vp, vp, vp]
    L.wrnn_generate.restype = i32
    L.wrnn_check.argtypes = [vp, vp]
    L.wrnn_check.restype = i32
    L.wrnn_elapsed_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.wrnn_elapsed_ms.restype = i32
    L.wrnn_query.argtypes = [vp, ctypes.POINTER(Info)]
    L.wrnn_query.restype = i32
    L.wrnn_last_error.argtypes = [vp]
    L.wrnn_last_error.restype = ctypes.c_char_p
    L.wrnn_destroy.argtypes = [vp]
    L.wrnn_destroy.restype = None
    pi = ctypes.POINTER(ctypes.c_int)
    L.wrnn_cond_shape.argtypes = [ctypes.POINTER(UpsampleCfg), i32, i32, i32, i32, pi, pi]
    L.wrnn_cond_shape.restype = i32
    L.wrnn_upsample_pack.argtypes = [ctypes.POINTER(UpsampleCfg), vp, vp, i32, i32, i32, i32, vp, vp]
    L.wrnn_upsample_pack.restype = i32
    L.wrnn_postprocess.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    L.wrnn_postprocess.restype = i32
    L.wrnn_generate_frames.argtypes = [vp, ctypes.POINTER(UpsampleCfg), vp, vp, i32, i32, i32, i32, vp, u64, i64, vp,
                                       vp, vp]
    L.wrnn_generate_frames.restype = i32
    L.wrnn_generate_frames_rows.argtypes = [vp, ctypes.POINTER(UpsampleCfg), vp, vp, i32, i32, i32, i32, i32, i32, vp,
                                            u64, i64, vp, vp, vp]
    L.wrnn_generate_frames_rows.restype = i32
    L.wrnn_frame_weights.argtypes = [ctypes.POINTER(UpsampleCfg), pi, pi, pi, vp, i32]
    L.wrnn_frame_weights.restype = i32
    L.wrnn_melresnet_floats.argtypes = [ctypes.POINTER(MelResNetCfg)]
    L.wrnn_melresnet_floats.restype = i32
    L.wrnn_melresnet.argtypes = [ctypes.POINTER(MelResNetCfg), vp, vp, i32, i32, vp, vp]
    L.wrnn_melresnet.restype = i32
    L.wrnn_melresnet_tile_frames.argtypes = [ctypes.POINTER(MelResNetCfg), i32, i32]
    L.wrnn_melresnet_tile_frames.restype = i32
    L.wrnn_philox_draws.argtypes = [u64, i64, i32, i32, i32, i32, i32, vp, vp]
    L.wrnn_philox_draws.restype = i32
    L.wrnn_stream_open.argtypes = [vp, ctypes.POINTER(UpsampleCfg), ctypes.POINTER(MelResNetCfg), vp, i32, i32, vp, i32,
                                   u64, i64, ctypes.POINTER(vp)]
    L.wrnn_stream_open.restype = i32
    L.wrnn_stream_open_wide.argtypes = L.wrnn_stream_open.argtypes
    L.wrnn_stream_open_wide.restype = i32
    L.wrnn_stream_open_rows.argtypes = L.wrnn_stream_open.argtypes
    L.wrnn_stream_open_rows.restype = i32
    # cfg, mel window (ptr, first frame, frames), aux window (ptr, first frame, frames), T (−1: unknown), U, t0, n, cond, stream
    L.wrnn_upsample_pack_window.argtypes = [ctypes.POINTER(UpsampleCfg), vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, vp,
                                            vp]
    L.wrnn_upsample_pack_window.restype = i32
    # cfg, T, t0, n → mel_lo, mel_hi, aux_lo, aux_hi
    L.wrnn_upsample_window_frames.argtypes = [ctypes.POINTER(UpsampleCfg), i32, i32, i32, pi, pi, pi, pi]
    L.wrnn_upsample_window_frames.restype = i32
    L.wrnn_stream_mu_law.argtypes = [vp, i32]
    L.wrnn_stream_mu_law.restype = i32
    L.wrnn_wide_steps_per_launch.argtypes = [i32, i32, i32]
    L.wrnn_wide_steps_per_launch.restype = i32
    # steps [count], rows [count], count, steps_per_launch → launch_first / launch_steps / launch_rows [cap], cap
    L.wrnn_wide_plan.argtypes = [pi, pi, i32, i32, pi, pi, pi, i32]
    L.wrnn_wide_plan.restype = i32
    L.wrnn_stream_push.argtypes = [vp, vp, i32, i32, vp, i32, pi, vp]
    L.wrnn_stream_push.restype = i32
    # arrays of `count` entries: sessions, mel pointers, n, final, wave pointers, cap, n_out
    L.wrnn_stream_push_group.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(vp), pi, pi, ctypes.POINTER(vp), pi, pi, vp]
    L.wrnn_stream_push_group.restype = i32
    L.wrnn_stream_plan.argtypes = [ctypes.POINTER(UpsampleCfg), i32, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.wrnn_stream_plan.restype = i32
    L.wrnn_stream_lookahead.argtypes = [ctypes.POINTER(UpsampleCfg)]
    L.wrnn_stream_lookahead.restype = i32
    L.wrnn_stream_close.argtypes = [vp]
    L.wrnn_stream_close.restype = None
    # frames [U], U, lanes → lane_of [U], pos_in_lane [U], lane_steps [lanes]
    L.wrnn_list_plan.argtypes = [pi, i32, i32, pi, pi, ctypes.POINTER(i64)]
    L.wrnn_list_plan.restype = i32
    # arrays of U entries: mel, aux pointers, T, (U, lanes), noise pointers (or NULL), seed, row_offset, out pointers
    L.wrnn_generate_list.argtypes = [vp, ctypes.POINTER(UpsampleCfg), ctypes.POINTER(vp), ctypes.POINTER(vp), pi, i32, i32,
                                     ctypes.POINTER(vp), u64, i64, ctypes.POINTER(vp), vp]
    L.wrnn_generate_list.restype = i32
    # frames [U], U, slots, hop, raw → slot_of [U], pos_in_slot [U], slot_frames [slots], launch_first / steps / rows [cap], cap
    L.wrnn_list_wide_plan.argtypes = [pi, i32, i32, i32, i32, pi, pi, ctypes.POINTER(i64), pi, pi, pi, i32]
    L.wrnn_list_wide_plan.restype = i32
    # wrnn_generate_list's arguments with slots (0: min(128, U)) in place of lanes
    L.wrnn_generate_list_wide.argtypes = L.wrnn_generate_list.argtypes
    L.wrnn_generate_list_wide.restype = i32
    # entries [U] (device), U, max_wave_len, mu_law, n_classes, fade_len, wave (device), stream
    L.wrnn_postprocess_list.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    L.wrnn_postprocess_list.restype = i32
    # frames [U], U, hop, target, overlap, slots, raw → folds [U], first_row [U], launch_first / steps / rows [cap], cap
    L.wrnn_list_folds_plan.argtypes = [pi, i32, i32, i32, i32, i32, i32, pi, pi, pi, pi, pi, i32]
    L.wrnn_list_folds_plan.restype = i32
    # wrnn_generate_list_wide's arguments with (target, overlap) before slots
    L.wrnn_generate_list_folds.argtypes = [vp, ctypes.POINTER(UpsampleCfg), ctypes.POINTER(vp), ctypes.POINTER(vp), pi, i32,
                                           i32, i32, i32, ctypes.POINTER(vp), u64, i64, ctypes.POINTER(vp), vp]
    L.wrnn_generate_list_folds.restype = i32
    # entries [U] (device), U, steps, overlap, max_wave_len, mu_law, n_classes, fade_len, wave (device), stream
    L.wrnn_postprocess_list_folds.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    L.wrnn_postprocess_list_folds.restype = i32
    L.wrnn_fingerprint.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i64), i32, vp, vp]
    L.wrnn_fingerprint.restype = i32
    pms, pi64 = ctypes.POINTER(MelSpecCfg), ctypes.POINTER(i64)
    L.wrnn_melspec_frames.argtypes = [pms, i64]
    L.wrnn_melspec_frames.restype = i64
    L.wrnn_melspec_table_floats.argtypes = [pms]
    L.wrnn_melspec_table_floats.restype = i32
    L.wrnn_melspec_tables.argtypes = [pms, vp]
    L.wrnn_melspec_tables.restype = i32
    # cfg, tables, wav pointers [U], n [U], U, mel pointers [U], ld [U], scratch, stream
    L.wrnn_melspec.argtypes = [pms, vp, ctypes.POINTER(vp), pi, i32, ctypes.POINTER(vp), pi, vp, vp]
    L.wrnn_melspec.restype = i32
    # cfg, tables, wav_tail, s0, ns, total (−1: unknown), t0, nt, mel, ld, scratch, stream
    L.wrnn_melspec_window.argtypes = [pms, vp, vp, i64, i32, i64, i32, i32, vp, i32, vp, vp]
    L.wrnn_melspec_window.restype = i32
    # the same with arrays of U entries (U after nt)
    L.wrnn_melspec_windows.argtypes = [pms, vp, ctypes.POINTER(vp), pi64, pi, pi64, pi, pi, i32, ctypes.POINTER(vp), pi,
                                       vp, vp]
    L.wrnn_melspec_windows.restype = i32
    # cfg, received, final → frames_ready, keep_from
    L.wrnn_melspec_plan.argtypes = [pms, i64, i32, pi64, pi64]
    L.wrnn_melspec_plan.restype = i32
    ptc, f32 = ctypes.POINTER(TacoCfg), ctypes.c_float
    L.wrnn_taco_supported.argtypes = [ptc]
    L.wrnn_taco_supported.restype = i32
    L.wrnn_taco_state_floats.argtypes = [ptc, i32]
    L.wrnn_taco_state_floats.restype = i32
    L.wrnn_taco_state_layout.argtypes = [ptc, i32, pi]
    L.wrnn_taco_state_layout.restype = i32
    L.wrnn_taco_scratch_floats.argtypes = [ptc, i32]
    L.wrnn_taco_scratch_floats.restype = i64
    # cfg, weights, enc, enc_proj, t_enc, t_max, rows, r, stop_threshold, step_cap, n_steps, state, mel, attn, scratch,
    # timeout_ms, stream
    L.wrnn_taco_run.argtypes = [ptc, ctypes.POINTER(TacoWeights), vp, vp, vp, i32, i32, i32, f32, i32, i32, vp, vp, vp, vp,
                                i32, vp]
    L.wrnn_taco_run.restype = i32
    pcc = ctypes.POINTER(CbhgCfg)
    L.wrnn_cbhg_supported.argtypes = [pcc]
    L.wrnn_cbhg_supported.restype = i32
    L.wrnn_cbhg_scratch_bytes.argtypes = [pcc, i64]
    L.wrnn_cbhg_scratch_bytes.restype = i64
    L.wrnn_cbhg_scratch_layout.argtypes = [pcc, i64, pi64]
    L.wrnn_cbhg_scratch_layout.restype = i32
    # cfg, weights, input (device), offsets (host, n_seq + 1), n_seq, out_rnn, out_proj, scratch, scratch_bytes, stream
    L.wrnn_cbhg_run.argtypes = [pcc, ctypes.POINTER(CbhgWeights), vp, pi, i32, vp, vp, vp, i64, vp]
    L.wrnn_cbhg_run.restype = i32
    L.wrnn_cond_last_error.argtypes = []
    L.wrnn_cond_last_error.restype = ctypes.c_char_p
    _lib = L
    return L


def check_cond(code: int):
    """Status of a stateless conditioning / post-processing call."""
    if code != 0:
        raise WrnnError(code, (lib().wrnn_cond_last_error() or b"").decode(errors="replace"))


def check(handle, code: int):
    if code != 0:
        msg = lib().wrnn_last_error(handle) if handle else b""
        raise (WrnnInvalid if code == -1 else WrnnError)(code, (msg or b"").decode(errors="replace"))
