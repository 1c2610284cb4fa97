"""ctypes binding of include/currennt_hip.h (one declaration per exported symbol)."""
import ctypes as C
import importlib.util
import os
import sys
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

PREC_F32, PREC_BF16, PREC_BF16X3 = 0, 1, 2
COMM_ID_BYTES = 128

# cn_layer_kind, keyed by the type strings of LayerFactory.cu:52-87
LAYER_KINDS = {
    "input": 0, "lstm": 1, "blstm": 2,
    "feedforward_tanh": 3, "feedforward_logistic": 4, "feedforward_identity": 5,
    "softmax": 6, "sse": 7, "multiclass_classification": 8,
    "weightedsse": 9, "wf": 10, "ce": 11, "rmse": 12, "binary_classification": 13,
    "ctc": 14,                # csrc/cn_ctc.hip; no counterpart in the reference
}
# CN_LAYER_CONTEXT, type string "context" (csrc/cn_context.hip): behind the kinds above in cn_layer_kind and no entry of the table,
# because cn_layer_create does not take it -- a context layer has members of its own and comes from cn_layer_create_context
KIND_CONTEXT = 15

# cn_buffer
BUF = {
    "outputs": 0, "outputErrors": 1, "weights": 2, "weightUpdates": 3, "weightDeltas": 4,
    "cellStates": 5, "niActs": 6, "igActs": 7, "fgActs": 8, "ogActs": 9,
    "niDeltas": 10, "igDeltas": 11, "fgDeltas": 12, "ogDeltas": 13, "tmpOutputs": 14,
    "adamSecondMoments": 15,
}

# every symbol include/currennt_hip.h declares (tests check the .so exports all of them)
EXPORTS = [
    "cn_ctx_create", "cn_ctx_destroy", "cn_ctx_synchronize", "cn_ctx_set_option", "cn_ctx_get_option", "cn_ctx_join", "cn_layer_join", "cn_layer_join_stream", "cn_ctx_stream", "cn_last_error", "cn_device_arch", "cn_device_count", "cn_device_name",
    "cn_version", "cn_layer_create", "cn_layer_destroy", "cn_layer_size", "cn_layer_kind_of",
    "cn_layer_weight_count", "cn_fraction_load", "cn_fraction_load_resident", "cn_fraction_prefetch_resident", "cn_fraction_prefetch", "cn_layer_forward",
    "cn_layer_backward", "cn_loss_eval", "cn_loss_accumulate", "cn_loss_read", "cn_layer_set_weights", "cn_layer_read", "cn_layer_write_output_errors", "cn_layer_upload",
    "cn_layer_device_ptr", "cn_ctx_param_arena", "cn_ctx_weights_touched", "cn_sgd_update",
    "cn_sgd_update_all", "cn_ctx_arm_update", "cn_ctx_accumulate_updates", "cn_ctx_take_accumulated", "cn_layer_set_learning_rate", "cn_ctx_timing_enable", "cn_ctx_timing_read", "cn_ctx_timing_reset",
    "cn_layer_recurrent_kernel",
    "cn_comm_unique_id", "cn_comm_init", "cn_comm_destroy", "cn_comm_info", "cn_comm_backend", "cn_allreduce_grads", "cn_loss_read_global",
    # include/currennt_hip_debug.h
    "cn_dbg_gemm_nt", "cn_dbg_gemm_tn", "cn_dbg_row_map_counts", "cn_dbg_prefetch_hits", "cn_dbg_gemm_tn_group", "cn_dbg_fold", "cn_dbg_layer_axis", "cn_dbg_layer_pad_bits",
    # the CTC post output layer: include/currennt_hip.h and its kernel-level hook in include/currennt_hip_debug.h
    "cn_layer_set_label_sequences", "cn_dbg_ctc",
    # include/currennt_hip.h, section Dropout, and its hook in include/currennt_hip_debug.h
    "cn_layer_set_dropout", "cn_ctx_set_dropout_pass", "cn_dbg_dropout_input",
    # include/currennt_hip.h, section Gradient clipping
    "cn_ctx_set_grad_clip", "cn_ctx_grad_clip_stats",
    # include/currennt_hip.h, section Weight noise, and its hook in include/currennt_hip_debug.h
    "cn_ctx_set_weight_noise", "cn_dbg_noisy_weights",
    # include/currennt_hip.h, section Input augmentation
    "cn_ctx_set_input_augment",
    # include/currennt_hip.h, section Input splicing and frame skipping
    "cn_ctx_set_input_splice",
    # include/currennt_hip.h, section Residual connections, and its hook in include/currennt_hip_debug.h
    "cn_layer_set_residual", "cn_dbg_residual_branch",
    # include/currennt_hip.h, section Layer normalization, and its hook in include/currennt_hip_debug.h
    "cn_layer_set_layer_norm", "cn_dbg_layer_norm_input",
    # include/currennt_hip.h, section Weight averaging
    "cn_ctx_average_weights", "cn_ctx_swap_weight_average", "cn_ctx_weight_average_state", "cn_layer_read_weight_average",
    "cn_layer_upload_weight_average",
    # include/currennt_hip.h, section Weight decay
    "cn_ctx_set_weight_decay", "cn_ctx_get_weight_decay",
    # include/currennt_hip.h, section Context layers
    "cn_layer_create_context", "cn_layer_context", "cn_layer_create_context_strided", "cn_layer_context_stride", "cn_layer_time",
    # include/currennt_hip.h, section LAMB
    "cn_lamb_update", "cn_lamb_update_all", "cn_ctx_arm_lamb", "cn_ctx_set_trust_bounds", "cn_ctx_get_trust_bounds", "cn_layer_trust_ratio",
    # include/currennt_hip.h, section CTC decoding, and its hook in include/currennt_hip_debug.h
    "cn_ctc_decode", "cn_ctc_decode_accumulate", "cn_ctc_decode_read", "cn_dbg_ctc_decode",
    # include/currennt_hip.h, section Adam (tests/test_adam_reference.py keeps this section last)
    "cn_adam_update", "cn_adam_update_all", "cn_ctx_arm_adam",
]


class CurrenntHipError(RuntimeError):
    """A non-zero cn_status; mirrors the reference's std::runtime_error (main.cpp:492-495)."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


class Fraction(C.Structure):
    _fields_ = [("max_seq_length", C.c_int), ("min_seq_length", C.c_int), ("num_sequences", C.c_int),
                ("input_pattern_size", C.c_int), ("output_pattern_size", C.c_int),
                ("pat_types", C.c_void_p), ("inputs", C.c_void_p),
                ("target_classes", C.c_void_p), ("targets", C.c_void_p)]


class InputAugment(C.Structure):
    """cn_input_augment (include/currennt_hip.h, section Input augmentation)"""
    _fields_ = [("noise_sigma", C.c_float), ("context_left", C.c_int), ("context_right", C.c_int),
                ("freq_masks", C.c_int), ("freq_width", C.c_int), ("time_masks", C.c_int), ("time_width", C.c_int),
                ("time_max_permille", C.c_int), ("seed", C.c_uint64), ("pass_", C.c_uint64)]


class InputSplice(C.Structure):
    """cn_input_splice (include/currennt_hip.h, section Input splicing and frame skipping)"""
    _fields_ = [("context_left", C.c_int), ("context_right", C.c_int), ("frame_skip", C.c_int)]


# include/currennt_hip_debug.h: cn_dbg_tn_item, cn_dbg_fold_item (every pointer a c_void_p: an int would be cut to 32 bits)
DBG_WS_SENTINEL = -1234.5
DBG_MAX_SPLITS = 8


class DbgTnItem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("rows_a", C.c_int), ("lda", C.c_int),
                ("B", C.c_void_p), ("rows_b", C.c_int), ("ldb", C.c_int),
                ("a_row", C.c_int), ("a_col", C.c_int), ("b_row", C.c_int), ("b_col", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("C", C.c_void_p), ("ldc", C.c_int)]


class DbgFoldItem(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("part", C.c_void_p), ("stride", C.c_longlong),
                ("nparts", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("ld", C.c_int),
                ("accumulate", C.c_int), ("clear", C.c_int)]


def lib_path():
    # CURRENNT_HIP_LIB: alternative build of the same library (A/B timing of two builds on one device)
    return os.environ.get("CURRENNT_HIP_LIB") or os.path.join(_HERE, "libcurrennt_hip.so")


def build_library(verbose=False):
    """hipcc --offload-arch=gfx950 build of csrc/ (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


def load_library():
    """Load libcurrennt_hip.so and declare the prototypes.  No fallback: a missing library is an error."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise CurrenntHipError(-5, "libcurrennt_hip.so is not built (run __graft_entry__.build()); "
                                   "there is no CPU fallback for the HIP path")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64, the library is linked against the system's.
    # Whichever is loaded first serves both (same SONAME); when the system's comes first, torch later reports
    # "No HIP GPUs are available".  So a process that can import torch loads torch's runtime before the library.
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None and not os.environ.get("CURRENNT_HIP_NO_TORCH_PRELOAD"):
        import torch  # noqa: F401
    L = C.CDLL(path)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.cn_ctx_create.argtypes = [ci, ci, vp, C.POINTER(vp)]
    L.cn_ctx_destroy.argtypes = [vp]
    L.cn_ctx_synchronize.argtypes = [vp]
    L.cn_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.cn_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    L.cn_ctx_join.argtypes = [vp]
    L.cn_layer_join.argtypes = [vp]
    L.cn_layer_join_stream.argtypes = [vp, vp]
    L.cn_ctx_stream.argtypes = [vp]
    L.cn_ctx_stream.restype = vp
    L.cn_last_error.argtypes = [vp]
    L.cn_last_error.restype = C.c_char_p
    L.cn_device_arch.argtypes = [vp]
    L.cn_device_arch.restype = C.c_char_p
    L.cn_device_count.argtypes = []
    L.cn_device_name.argtypes = [ci, C.c_char_p, ci]
    L.cn_version.restype = C.c_char_p
    L.cn_layer_create.argtypes = [vp, ci, vp, ci, cf, ci, ci, C.POINTER(vp)]
    L.cn_layer_destroy.argtypes = [vp]
    L.cn_layer_size.argtypes = [vp]
    L.cn_layer_kind_of.argtypes = [vp]
    L.cn_layer_weight_count.argtypes = [vp]
    L.cn_fraction_load.argtypes = [vp, vp, vp, C.POINTER(Fraction)]
    L.cn_fraction_load_resident.argtypes = [vp, vp, vp, C.POINTER(Fraction)]
    L.cn_fraction_prefetch_resident.argtypes = [vp, vp, vp, C.POINTER(Fraction)]
    L.cn_fraction_prefetch.argtypes = [vp, vp, vp, C.POINTER(Fraction)]
    L.cn_loss_accumulate.argtypes = [vp]
    L.cn_loss_read.argtypes = [vp, C.POINTER(cf), C.POINTER(C.c_int64), ci]
    L.cn_layer_forward.argtypes = [vp]
    L.cn_layer_backward.argtypes = [vp]
    L.cn_loss_eval.argtypes = [vp, C.POINTER(cf), C.POINTER(ci)]
    L.cn_layer_set_weights.argtypes = [vp, vp, ci]
    L.cn_layer_read.argtypes = [vp, ci, ci, vp, C.c_size_t]
    L.cn_layer_write_output_errors.argtypes = [vp, vp, C.c_size_t]
    L.cn_layer_upload.argtypes = [vp, ci, vp, C.c_size_t]
    L.cn_layer_device_ptr.argtypes = [vp, ci]
    L.cn_layer_device_ptr.restype = vp
    L.cn_ctx_param_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.cn_ctx_weights_touched.argtypes = [vp]
    L.cn_sgd_update.argtypes = [vp, cf, cf]
    L.cn_sgd_update_all.argtypes = [vp, cf, cf]
    L.cn_ctx_arm_update.argtypes = [vp, cf, cf]
    L.cn_adam_update.argtypes = [vp, cf, cf, cf, cf, C.c_int64]
    L.cn_adam_update_all.argtypes = [vp, cf, cf, cf, cf, C.c_int64]
    L.cn_ctx_arm_adam.argtypes = [vp, cf, cf, cf, cf, C.c_int64]
    L.cn_lamb_update.argtypes = [vp, cf, cf, cf, cf, C.c_int64]
    L.cn_lamb_update_all.argtypes = [vp, cf, cf, cf, cf, C.c_int64]
    L.cn_ctx_arm_lamb.argtypes = [vp, cf, cf, cf, cf, C.c_int64]
    L.cn_ctx_set_trust_bounds.argtypes = [vp, cf, cf]
    L.cn_ctx_get_trust_bounds.argtypes = [vp, C.POINTER(cf), C.POINTER(cf)]
    L.cn_layer_trust_ratio.argtypes = [vp, C.POINTER(cf), C.POINTER(cf), C.POINTER(cf)]
    L.cn_ctx_accumulate_updates.argtypes = [vp, ci]
    L.cn_ctx_take_accumulated.argtypes = [vp]
    L.cn_ctx_timing_enable.argtypes = [vp, ci]
    L.cn_ctx_timing_read.argtypes = [vp, ci, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.cn_ctx_timing_reset.argtypes = [vp]
    L.cn_layer_set_learning_rate.argtypes = [vp, cf]
    L.cn_layer_recurrent_kernel.argtypes = [vp, ci]
    L.cn_layer_recurrent_kernel.restype = C.c_char_p
    L.cn_comm_unique_id.argtypes = [C.c_char_p]
    L.cn_comm_init.argtypes = [vp, C.c_char_p, ci, ci]
    L.cn_comm_destroy.argtypes = [vp]
    L.cn_comm_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.cn_comm_backend.argtypes = [vp, C.POINTER(C.c_int64)]
    L.cn_comm_backend.restype = C.c_char_p
    L.cn_allreduce_grads.argtypes = [vp, C.POINTER(vp), ci]
    L.cn_loss_read_global.argtypes = [vp, C.POINTER(cf), C.POINTER(C.c_int64), ci]
    L.cn_dbg_gemm_nt.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, ci]
    L.cn_dbg_gemm_tn.argtypes = [vp, vp, vp, vp, ci, ci, ci]
    L.cn_dbg_gemm_tn_group.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.cn_dbg_fold.argtypes = [vp, vp, ci]
    L.cn_dbg_row_map_counts.argtypes = [vp, vp]
    L.cn_dbg_prefetch_hits.argtypes = [vp, C.POINTER(C.c_int)]
    L.cn_layer_set_label_sequences.argtypes = [vp, vp, vp, ci]
    L.cn_dbg_ctc.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]
    L.cn_ctc_decode.argtypes = [vp, vp, vp, vp]
    L.cn_ctc_decode_accumulate.argtypes = [vp]
    L.cn_ctc_decode_read.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), ci]
    L.cn_dbg_ctc_decode.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp]
    L.cn_layer_set_dropout.argtypes = [vp, cf]
    L.cn_ctx_set_dropout_pass.argtypes = [vp, ci, C.c_uint64, C.c_uint64]
    L.cn_dbg_dropout_input.argtypes = [vp, vp, C.c_size_t]
    L.cn_layer_set_residual.argtypes = [vp, ci]
    L.cn_dbg_residual_branch.argtypes = [vp, vp, C.c_size_t]
    L.cn_layer_set_layer_norm.argtypes = [vp, ci, cf]
    L.cn_dbg_layer_norm_input.argtypes = [vp, vp, C.c_size_t]
    L.cn_ctx_set_grad_clip.argtypes = [vp, cf]
    L.cn_ctx_grad_clip_stats.argtypes = [vp, C.POINTER(cf), C.POINTER(cf), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(cf), ci]
    L.cn_ctx_set_weight_decay.argtypes = [vp, cf]
    L.cn_ctx_get_weight_decay.argtypes = [vp, C.POINTER(cf)]
    L.cn_ctx_set_weight_noise.argtypes = [vp, cf, C.c_uint64, C.c_uint64]
    L.cn_dbg_noisy_weights.argtypes = [vp, vp, C.c_size_t]
    L.cn_ctx_set_input_augment.argtypes = [vp, C.POINTER(InputAugment)]
    L.cn_ctx_set_input_splice.argtypes = [vp, C.POINTER(InputSplice)]
    L.cn_ctx_average_weights.argtypes = [vp, cf]
    L.cn_ctx_swap_weight_average.argtypes = [vp]
    L.cn_ctx_weight_average_state.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.cn_layer_read_weight_average.argtypes = [vp, vp, C.c_size_t]
    L.cn_layer_upload_weight_average.argtypes = [vp, vp, C.c_size_t]
    L.cn_layer_create_context.argtypes = [vp, vp, ci, ci, ci, C.POINTER(vp)]
    L.cn_layer_context.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.cn_layer_create_context_strided.argtypes = [vp, vp, ci, ci, ci, ci, C.POINTER(vp)]
    L.cn_layer_context_stride.argtypes = [vp, C.POINTER(ci)]
    L.cn_layer_time.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.cn_dbg_layer_axis.argtypes = [vp, vp, vp, vp, C.c_size_t, C.POINTER(ci)]
    L.cn_dbg_layer_pad_bits.argtypes = [vp, C.POINTER(C.c_longlong)]
    _LIB = L
    return L


def check(rc, ctx=None):
    if rc != 0:
        msg = load_library().cn_last_error(ctx)
        raise CurrenntHipError(rc, msg.decode() if msg else "cn_status %d" % rc)
