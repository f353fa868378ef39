"""ctypes binding of libnfp_hip.so — the C ABI declared in include/nfp.h.

This is the whole boundary between Python and the HIP kernels: plain pointers,
sizes and one descriptor struct.  There is no CPU implementation behind it; if
the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnfp_hip.so")
ABI_VERSION = 7

MEASURES = ["norm", "cosine", "dot", "rmse", "geman", "attention", "emd", "canberra", "hellinger",
            "chisquared1", "chisquared2", "gfc", "pearson", "jeffrey", "squaredchord", "smith", "scs"]
MEASURE_ALIASES = {"sharpened_cosine": "scs"}
PAD_MODES = ["zeros", "reflect", "replicate", "circular"]
F32, BF16 = 0, 1
TICKET_BYTES = 4096 * 4       # the arrival counters at the head of a workspace (csrc/nfp_common.h: kTicketBytes)

EXPORTS = ["nfp_abi_version", "nfp_last_error", "nfp_output_shape", "nfp_saved_floats", "nfp_forward",
           "nfp_backward", "nfp_pool_supported", "nfp_pool_saved_floats", "nfp_pool_forward", "nfp_pool_backward", "nfp_launch_count",
           "nfp_last_variant", "nfp_plan", "nfp_reload_env", "nfp_workspace_bytes", "nfp_workspace_init", "nfp_time_next_launch",
           "nfp_bias_saved_floats", "nfp_bias_scratch_floats", "nfp_bias_forward", "nfp_bias_backward",
           "nfp_gap_supported", "nfp_gap_saved_floats", "nfp_gap_forward", "nfp_gap_backward",
           "nfp_attpool_scratch_floats", "nfp_attpool_forward", "nfp_attpool_backward",
           "nfp_deepten_saved_floats", "nfp_deepten_scratch_floats", "nfp_deepten_forward", "nfp_deepten_backward",
           "nfp_valid_supported", "nfp_valid_saved_floats", "nfp_valid_forward", "nfp_valid_backward",
           "nfp_valid_abs_supported", "nfp_valid_abs_forward", "nfp_valid_abs_backward",
           "nfp_strided_supported", "nfp_strided_saved_floats", "nfp_strided_forward", "nfp_strided_backward",
           "nfp_cpool_saved_floats", "nfp_cpool_scratch_floats", "nfp_cpool_forward", "nfp_cpool_backward",
           "nfp_cproj_scratch_floats", "nfp_cproj_forward", "nfp_cproj_backward",
           "nfp_cproj_forward_fmt", "nfp_cproj_backward_fmt",
           "nfp_cpool_wide_scratch_floats", "nfp_cpool_wide_forward", "nfp_cpool_wide_backward",
           "nfp_cpsync_record_doubles", "nfp_cpsync_kq_floats", "nfp_cpsync_saved_floats", "nfp_cpsync_moments",
           "nfp_cpsync_forward", "nfp_cpsync_reduce", "nfp_cpsync_maps"]
ACT_NCHW, ACT_NHWC = 0, 1     # enum nfp_act_layout: out / grad_out of nfp_cproj_*_fmt
CP_POOL, CP_PROJ = 0, 1       # enum nfp_cp_kind: the first argument of nfp_cpsync_forward / _reduce / _maps


class NfpDesc(ctypes.Structure):
    """struct nfp_desc (include/nfp.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("B", "C", "H", "W", "R", "pad", "stride", "dilation", "pad_mode", "measure",
                 "similarity", "diff_weights", "dtype")] + \
               [("p", ctypes.c_float), ("eps", ctypes.c_float), ("q_scs", ctypes.c_float)] + \
               [(n, ctypes.c_int64) for n in ("sxB", "sxC", "sxH", "sxW", "sgB")] + [("ws", ctypes.c_void_p), ("inner_R", ctypes.c_int32), ("map_f32", ctypes.c_int32)]


class NfpError(RuntimeError):
    pass


class NfpUnsupported(NfpError, NotImplementedError):
    pass


_lib = None


def load():
    """Load libnfp_hip.so (once).  Raises NfpError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NfpError(
            f"{LIB_PATH} is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `python -m neighbour_feature_pooling_amd.build`). There is no fallback for GPU tensors.")
    L = ctypes.CDLL(LIB_PATH)
    vp, dp = ctypes.c_void_p, ctypes.POINTER(NfpDesc)
    i32p = ctypes.POINTER(ctypes.c_int32)
    L.nfp_abi_version.restype = ctypes.c_int
    L.nfp_last_error.restype = ctypes.c_char_p
    L.nfp_last_variant.restype = ctypes.c_char_p
    L.nfp_launch_count.restype = ctypes.c_uint64
    L.nfp_reload_env.restype = None
    L.nfp_time_next_launch.argtypes = [vp, vp]
    L.nfp_time_next_launch.restype = None
    L.nfp_plan.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]
    L.nfp_plan.restype = ctypes.c_int
    L.nfp_output_shape.argtypes = [dp, i32p, i32p, i32p]
    L.nfp_saved_floats.argtypes = [dp]
    L.nfp_saved_floats.restype = ctypes.c_int64
    L.nfp_workspace_bytes.argtypes = [dp]
    L.nfp_workspace_bytes.restype = ctypes.c_int64
    L.nfp_workspace_init.argtypes = [dp, vp, vp]
    L.nfp_forward.argtypes = [dp, vp, vp, vp, vp]
    L.nfp_backward.argtypes = [dp, vp, vp, vp, vp, vp, vp]
    L.nfp_pool_supported.argtypes = [dp]
    if hasattr(L, "nfp_pool_saved_floats"):     # (absent only from an older library loaded for an A/B run)
        L.nfp_pool_saved_floats.argtypes = [dp]
        L.nfp_pool_saved_floats.restype = ctypes.c_int64
    L.nfp_pool_forward.argtypes = [dp, vp, vp, vp, vp, vp, vp]
    L.nfp_pool_backward.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp]
    i64 = ctypes.c_int64
    L.nfp_bias_saved_floats.argtypes = [dp]
    L.nfp_bias_saved_floats.restype = i64
    L.nfp_bias_scratch_floats.argtypes = [dp]
    L.nfp_bias_scratch_floats.restype = i64
    L.nfp_bias_forward.argtypes = [dp, vp, vp, vp, vp, vp, i64, vp]
    L.nfp_bias_backward.argtypes = [dp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    if hasattr(L, "nfp_gap_forward"):           # (absent only from an older library loaded for an A/B run)
        L.nfp_gap_supported.argtypes = [dp]
        L.nfp_gap_saved_floats.argtypes = [dp]
        L.nfp_gap_saved_floats.restype = i64
        L.nfp_gap_forward.argtypes = [dp, vp, vp, vp, vp, i64, vp]
        L.nfp_gap_backward.argtypes = [dp, vp, vp, vp, vp, vp, i64, vp, vp]
    if hasattr(L, "nfp_attpool_forward"):       # (absent only from an older library loaded for an A/B run)
        i32 = ctypes.c_int32
        L.nfp_attpool_scratch_floats.argtypes = [i32, i32]
        L.nfp_attpool_scratch_floats.restype = i64
        L.nfp_attpool_forward.argtypes = [i32, i32, i64, i32, vp, vp, vp, vp, vp, vp]
        L.nfp_attpool_backward.argtypes = [i32, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    if hasattr(L, "nfp_deepten_forward"):       # (absent only from an older library loaded for an A/B run)
        i32 = ctypes.c_int32
        L.nfp_deepten_saved_floats.argtypes = [i32, i64, i32]
        L.nfp_deepten_scratch_floats.argtypes = [i32, i64, i32, i32, i32]
        L.nfp_deepten_saved_floats.restype = L.nfp_deepten_scratch_floats.restype = i64
        head = [i32, i64, i32, i32, i32, i32, i64, vp, vp, vp]          # B, N, K, D, dtype, layout, sxB, x, codewords, scale
        L.nfp_deepten_forward.argtypes = head + [vp, vp, i64, vp]
        L.nfp_deepten_backward.argtypes = head + [vp, i64, vp, vp, vp, vp, vp, i64, vp]
    if hasattr(L, "nfp_valid_forward"):         # (absent only from an older library loaded for an A/B run)
        L.nfp_valid_supported.argtypes = [dp]
        L.nfp_valid_saved_floats.argtypes = [dp]
        L.nfp_valid_saved_floats.restype = i64
        L.nfp_valid_forward.argtypes = [dp, vp, vp, vp, i64, vp]
        L.nfp_valid_backward.argtypes = [dp, vp, vp, vp, vp, i64, vp, vp]
    if hasattr(L, "nfp_strided_forward"):       # (absent only from an older library loaded for an A/B run)
        L.nfp_strided_supported.argtypes = [dp]
        L.nfp_strided_saved_floats.argtypes = [dp]
        L.nfp_strided_saved_floats.restype = i64
        L.nfp_strided_forward.argtypes = [dp, vp, vp, vp, i64, vp]
        L.nfp_strided_backward.argtypes = [dp, vp, vp, vp, vp, i64, vp, vp]
    if hasattr(L, "nfp_valid_abs_forward"):     # (absent only from an older library loaded for an A/B run)
        L.nfp_valid_abs_supported.argtypes = [dp]
        L.nfp_valid_abs_forward.argtypes = [dp, vp, vp, vp]
        L.nfp_valid_abs_backward.argtypes = [dp, vp, vp, vp, vp]
    if hasattr(L, "nfp_cpool_forward"):         # (absent only from an older library loaded for an A/B run)
        i32, f64 = ctypes.c_int32, ctypes.c_double
        L.nfp_cpool_saved_floats.argtypes = [i32, i32]
        L.nfp_cpool_saved_floats.restype = i64
        L.nfp_cpool_scratch_floats.argtypes = [i32, i32, i64, i32, i32]
        L.nfp_cpool_scratch_floats.restype = i64
        L.nfp_cpool_forward.argtypes = [i32, i32, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, f64, f64, vp, vp, i64, vp, i64, vp]
        L.nfp_cpool_backward.argtypes = [i32, i32, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, f64, vp, i64, vp, vp, vp, vp,
                                         vp, vp, i64, vp]
    if hasattr(L, "nfp_cproj_forward"):         # (absent only from an older library loaded for an A/B run)
        L.nfp_cproj_scratch_floats.argtypes = [i32, i32, i64, i32, i32]
        L.nfp_cproj_scratch_floats.restype = i64
        L.nfp_cproj_forward.argtypes = [i32, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f64, f64, vp, vp, i64, vp, i64,
                                        vp]
        L.nfp_cproj_backward.argtypes = [i32, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f64, vp, i64, vp, vp, vp, vp,
                                         vp, vp, i64, vp]
    if hasattr(L, "nfp_cproj_forward_fmt"):     # (absent only from an older library loaded for an A/B run)
        L.nfp_cproj_forward_fmt.argtypes = L.nfp_cproj_forward.argtypes + [i32]
        L.nfp_cproj_backward_fmt.argtypes = L.nfp_cproj_backward.argtypes + [i32]
    if hasattr(L, "nfp_cpool_wide_forward"):    # (absent only from an older library loaded for an A/B run)
        L.nfp_cpool_wide_scratch_floats.argtypes = L.nfp_cpool_scratch_floats.argtypes
        L.nfp_cpool_wide_scratch_floats.restype = i64
        L.nfp_cpool_wide_forward.argtypes = L.nfp_cpool_forward.argtypes
        L.nfp_cpool_wide_backward.argtypes = L.nfp_cpool_backward.argtypes
    if hasattr(L, "nfp_cpsync_forward"):        # (absent only from an older library loaded for an A/B run)
        i32, f64 = ctypes.c_int32, ctypes.c_double
        L.nfp_cpsync_record_doubles.argtypes = L.nfp_cpsync_kq_floats.argtypes = [i32]
        L.nfp_cpsync_saved_floats.argtypes = [i32, i32]
        L.nfp_cpsync_record_doubles.restype = L.nfp_cpsync_kq_floats.restype = L.nfp_cpsync_saved_floats.restype = i64
        L.nfp_cpsync_moments.argtypes = [i32, i32, i64, i32, vp, vp, i64, vp, i64, vp]
        head = [i32, i32, i32, i64, i32, i32, i32, vp, vp, vp, vp]      # kind, B, N, P, D, dtype, relu, maps, w, gamma, beta
        L.nfp_cpsync_forward.argtypes = head + [vp, vp, f64, f64, vp, i32, i64, i64, vp, vp, i64, vp, i32]
        L.nfp_cpsync_reduce.argtypes = head + [f64, vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, i32]
        L.nfp_cpsync_maps.argtypes = head + [f64, vp, i64, vp, vp, i32, i64, vp, vp, i32]
    if L.nfp_abi_version() != ABI_VERSION:
        raise NfpError(f"libnfp_hip.so ABI {L.nfp_abi_version()} != binding {ABI_VERSION}; rebuild")
    _lib = L
    return L


def check(rc):
    if rc == 0:
        return
    msg = load().nfp_last_error().decode()
    if rc == -2:
        raise NfpUnsupported(f"libnfp_hip: {msg}")
    raise NfpError(f"libnfp_hip rc={rc}: {msg}")


def measure_id(name):
    name = MEASURE_ALIASES.get(name, name)
    return MEASURES.index(name)
