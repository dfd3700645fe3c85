"""ctypes binding of libtadmm_hip.so (include/tadmm.h).

The library is the product; there is no CPU fallback.  ``load()`` raises
``TadmmLibraryError`` when the shared object is missing or does not export the
full C ABI, and every compute wrapper raises ``TadmmError`` when the C side
returns a negative status (with ``tadmm_last_error`` text).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

MAX_MODES = 8

KIND_TT_CONV, KIND_TT_LINEAR, KIND_SVD, KIND_TUCKER2 = 0, 1, 2, 3
FLAG_SKIP_ROTATIONS = 1

_LIB_NAME = "libtadmm_hip.so"
_HERE = os.path.dirname(os.path.abspath(__file__))


class TadmmLibraryError(RuntimeError):
    pass


class TadmmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"tadmm status {status}: {msg}")
        self.status = status


class LayerDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("ndim", C.c_int32),
        ("dims", C.c_int64 * 4),
        ("d", C.c_int32),
        ("tt_shapes", C.c_int32 * MAX_MODES),
        ("ranks", C.c_int32 * (MAX_MODES + 1)),
        ("flags", C.c_uint32),
        ("hooi_max_iter", C.c_int32),
        ("hooi_tol", C.c_float),
    ]


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("a_rs", C.c_int64), ("a_cs", C.c_int64),
        ("b_rs", C.c_int64), ("b_cs", C.c_int64),
        ("c_rs", C.c_int64), ("c_cs", C.c_int64),
        ("alpha", C.c_float), ("beta", C.c_float),
        ("bias_n", C.c_void_p), ("bias_m", C.c_void_p),
    ]


class ChainDesc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("Y", C.c_void_p), ("Win", C.c_void_p), ("Wout", C.c_void_p), ("bias", C.c_void_p),
        ("T", C.c_int64),
        ("Kin", C.c_int32), ("R", C.c_int32), ("Nout", C.c_int32),
        ("ldx", C.c_int64), ("ldy", C.c_int64), ("win_plane", C.c_int64), ("wout_plane", C.c_int64),
        ("x_hw", C.c_int32), ("y_hw", C.c_int32), ("dtype", C.c_int32), ("tile_tokens", C.c_int32),
    ]


class ConvChainDesc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("Y", C.c_void_p), ("W1", C.c_void_p), ("W2", C.c_void_p), ("W3", C.c_void_p),
        ("bias", C.c_void_p),
        ("w1_plane", C.c_int64), ("w2_plane", C.c_int64), ("w3_plane", C.c_int64),
        ("B", C.c_int32), ("C", C.c_int32), ("R1", C.c_int32), ("R2", C.c_int32), ("Nout", C.c_int32),
        ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
        ("stride_h", C.c_int32), ("stride_w", C.c_int32), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("dil_h", C.c_int32), ("dil_w", C.c_int32), ("dtype", C.c_int32),
    ]


CHAIN_F32, CHAIN_BF16, CHAIN_F16 = 0, 1, 2    # F16: inference entries only (include/tadmm.h)
CONV_CHAIN_FWD, CONV_CHAIN_BWD = 0, 1


class OrthDesc(C.Structure):
    _fields_ = [
        ("P", C.c_void_p), ("grad_offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32),
        ("ld", C.c_int64), ("gram_of_rows", C.c_int32), ("reserved", C.c_int32),
    ]


class StiefelDesc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("G", C.c_void_p), ("M", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32),
        ("ld", C.c_int64),
    ]


BERTADAM_CHUNK = 4096    # kBaChunk of csrc/bertadam.hip (checked against the library at load)


class BertAdamDesc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class DgemmTileProb(C.Structure):
    """tadmm_dgemm_tile_prob: one problem of the filter's tile product / daxpby as the filter describes it (tests)."""
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("P", C.c_void_p), ("Q", C.c_void_p),
        ("ring", C.c_void_p * 3), ("rot", C.c_void_p),
        ("selA", C.c_int32), ("selB", C.c_int32), ("selC", C.c_int32), ("selP", C.c_int32), ("selQ", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
        ("mode", C.c_int32),
        ("coef", C.c_void_p), ("theta", C.c_void_p), ("rowpart", C.c_void_p),
        ("gate", C.c_void_p), ("gate_min", C.c_int32),
    ]


class TileMapProb(C.Structure):
    """tadmm_tile_map_prob: sizes and tile shape of one problem of a grouped tile product (host-only map builder)."""
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("tile_m", C.c_int32), ("tile_n", C.c_int32)]


TTM_MAX_D = 4


class TtmDesc(C.Structure):
    _fields_ = [
        ("cores", C.c_void_p * TTM_MAX_D), ("dcores", C.c_void_p * TTM_MAX_D),
        ("order", C.c_void_p * TTM_MAX_D), ("offsets", C.c_void_p * TTM_MAX_D),
        ("index", C.c_void_p), ("dY", C.c_void_p), ("Y", C.c_void_p), ("bad_count", C.c_void_p),
        ("B", C.c_int64), ("d", C.c_int32), ("index_dtype", C.c_int32),
        ("n", C.c_int32 * TTM_MAX_D), ("m", C.c_int32 * TTM_MAX_D), ("r", C.c_int32 * (TTM_MAX_D + 1)),
        ("reserved", C.c_int32),
    ]


class LstmDesc(C.Structure):
    _fields_ = [
        ("Xp", C.c_void_p), ("W", C.c_void_p), ("h0", C.c_void_p), ("c0", C.c_void_p),
        ("Y", C.c_void_p), ("hT", C.c_void_p), ("cT", C.c_void_p), ("G", C.c_void_p), ("C", C.c_void_p),
        ("dY", C.c_void_p), ("dhT", C.c_void_p), ("dcT", C.c_void_p),
        ("dZ", C.c_void_p), ("dh0", C.c_void_p), ("dc0", C.c_void_p),
        ("T", C.c_int64), ("B", C.c_int64), ("H", C.c_int32), ("sigmoid", C.c_int32),
    ]


DISTILL_BASE_NONE, DISTILL_BASE_INDEX, DISTILL_BASE_DENSE = 0, 1, 2
DISTILL_KD_NONE, DISTILL_KD_SOFT_KL, DISTILL_KD_HARD, DISTILL_KD_SOFT_CE = 0, 1, 2, 3


class DistillDesc(C.Structure):
    _fields_ = [
        ("s", C.c_void_p), ("k", C.c_void_p), ("t", C.c_void_p),
        ("s_ld", C.c_int64), ("k_ld", C.c_int64), ("t_ld", C.c_int64),
        ("labels", C.c_void_p), ("dense", C.c_void_p), ("dense_ld", C.c_int64),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("loss_dev", C.c_void_p), ("loss_f32_dev", C.c_void_p), ("counts_dev", C.c_void_p),
        ("grad_s", C.c_void_p), ("grad_k", C.c_void_p),
        ("ignore_index", C.c_int64),
        ("eps", C.c_double), ("alpha", C.c_double), ("tau", C.c_double),
        ("B", C.c_int32), ("C", C.c_int32), ("dtype", C.c_int32),
        ("base_kind", C.c_int32), ("kd_kind", C.c_int32), ("reserved", C.c_int32),
    ]


LAYER_MSE_MAX_PAIRS = 32
LAYER_MSE_ATT, LAYER_MSE_REP = 0, 1


class LayerMsePair(C.Structure):
    _fields_ = [
        ("s", C.c_void_p), ("t", C.c_void_p), ("grad", C.c_void_p),
        ("n", C.c_int64), ("scale", C.c_double), ("thr", C.c_float),
        ("clamp", C.c_int32), ("group", C.c_int32), ("reserved", C.c_int32),
    ]


class LayerMseDesc(C.Structure):
    _fields_ = [
        ("pairs", LayerMsePair * LAYER_MSE_MAX_PAIRS),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("terms_dev", C.c_void_p), ("loss_dev", C.c_void_p), ("loss_f32_dev", C.c_void_p),
        ("npairs", C.c_int32), ("dtype", C.c_int32),
    ]


class AttnDesc(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p),
        ("q_ld", C.c_int64), ("k_ld", C.c_int64), ("v_ld", C.c_int64),
        ("q_bs", C.c_int64), ("k_bs", C.c_int64), ("v_bs", C.c_int64),
        ("mask", C.c_void_p), ("keep", C.c_void_p),
        ("ctx", C.c_void_p), ("scores", C.c_void_p), ("stats", C.c_void_p),
        ("g_ctx", C.c_void_p), ("g_sc", C.c_void_p),
        ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("p", C.c_double),
        ("B", C.c_int64), ("H", C.c_int32), ("S", C.c_int32), ("d", C.c_int32), ("dtype", C.c_int32),
    ]


class BertNormDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("res", C.c_void_p),
        ("x_ld", C.c_int64), ("res_ld", C.c_int64),
        ("keep", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("y", C.c_void_p), ("stats", C.c_void_p), ("g", C.c_void_p),
        ("dx", C.c_void_p), ("dres", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("p", C.c_double), ("eps", C.c_double),
        ("rows", C.c_int64), ("hidden", C.c_int32), ("dtype", C.c_int32), ("param_dtype", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PreNormDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("b", C.c_void_p),
        ("x_ld", C.c_int64), ("b_ld", C.c_int64),
        ("keep", C.c_void_p), ("path_keep", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("s", C.c_void_p), ("y", C.c_void_p), ("stats", C.c_void_p), ("g_y", C.c_void_p), ("g_s", C.c_void_p),
        ("dx", C.c_void_p), ("db", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("p", C.c_double), ("p_path", C.c_double), ("eps", C.c_double),
        ("rows", C.c_int64), ("rows_per_sample", C.c_int64),
        ("hidden", C.c_int32), ("dtype", C.c_int32), ("param_dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class BnActDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("res", C.c_void_p), ("res_stride", C.c_int64 * 4),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
        ("num_batches_tracked", C.c_void_p),
        ("y", C.c_void_p), ("stats", C.c_void_p), ("g", C.c_void_p),
        ("dx", C.c_void_p), ("dres", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("eps", C.c_double), ("momentum", C.c_double),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("c0", C.c_int32), ("Cr", C.c_int32),
        ("dtype", C.c_int32), ("training", C.c_int32), ("relu", C.c_int32), ("reserved", C.c_int32),
    ]


class DwBnDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p),
        ("z", C.c_void_p), ("y", C.c_void_p), ("stats", C.c_void_p), ("g", C.c_void_p),
        ("dx", C.c_void_p), ("dw", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("eps", C.c_double), ("momentum", C.c_double),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32),
        ("dtype", C.c_int32), ("training", C.c_int32), ("reserved", C.c_int32),
    ]


DENSEBN_MAX_SEGMENTS = 128                  # TADMM_DENSEBN_MAX_SEGMENTS


class DenseBnSeg(C.Structure):
    _fields_ = [("x", C.c_void_p), ("stats", C.c_void_p), ("dx", C.c_void_p), ("C", C.c_int32), ("reserved", C.c_int32)]


class DenseBnDesc(C.Structure):
    _fields_ = [
        ("seg", DenseBnSeg * DENSEBN_MAX_SEGMENTS),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
        ("num_batches_tracked", C.c_void_p),
        ("y", C.c_void_p), ("g", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("eps", C.c_double), ("momentum", C.c_double),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("nseg", C.c_int32),
        ("dtype", C.c_int32), ("training", C.c_int32), ("relu", C.c_int32), ("reserved", C.c_int32),
    ]


class WgradDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
        ("T", C.c_int64), ("M", C.c_int32), ("N", C.c_int32),
        ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64),
        ("hw", C.c_int32), ("dtype", C.c_int32), ("alpha", C.c_float), ("reserved", C.c_int32),
    ]


class CoreConvDesc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("Y", C.c_void_p), ("Wc", C.c_void_p), ("wc_plane", C.c_int64),
        ("B", C.c_int32), ("R1", C.c_int32), ("R2", C.c_int32),
        ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
        ("stride_h", C.c_int32), ("stride_w", C.c_int32), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("dil_h", C.c_int32), ("dil_w", C.c_int32), ("dtype", C.c_int32),
    ]


# name -> (restype, argtypes); this table IS the list of symbols include/tadmm.h declares
ABI = {
    "tadmm_version": (C.c_int, []),
    "tadmm_abi_sizes": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tadmm_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "tadmm_destroy": (C.c_int, [C.c_void_p]),
    "tadmm_last_error": (C.c_char_p, [C.c_void_p]),
    "tadmm_tt_clamp_ranks": (C.c_int, [C.POINTER(LayerDesc)]),
    "tadmm_plan_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LayerDesc), C.POINTER(C.c_size_t)]),
    "tadmm_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LayerDesc), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "tadmm_plan_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tadmm_plan_singular_values": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "tadmm_plan_last_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "tadmm_plan_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "tadmm_plan_set_jacobi": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int]),
    "tadmm_plan_filter_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "tadmm_plan_filter_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "tadmm_plan_filter_timing_fast": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "tadmm_plan_jacobi_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "tadmm_plan_ranks": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "tadmm_plan_lanes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "tadmm_lane_split": (C.c_int, [C.c_int, C.POINTER(LayerDesc), C.POINTER(C.c_int32)]),
    "tadmm_plan_destroy": (C.c_int, [C.c_void_p]),
    "tadmm_tucker_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LayerDesc), C.POINTER(C.c_size_t)]),
    "tadmm_tucker_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LayerDesc), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_void_p)]),
    "tadmm_tucker_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tadmm_tucker_factors": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p)]),
    "tadmm_tucker_jacobi_sweeps": (C.c_int, [C.c_void_p]),
    "tadmm_tucker_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "tadmm_tucker_last_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "tadmm_tucker_iterations": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p]),
    "tadmm_tucker_destroy": (C.c_int, [C.c_void_p]),
    "tadmm_penalty_scratch_doubles": (C.c_int, []),
    "tadmm_penalty": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "tadmm_orth_desc_bytes": (C.c_int, []),
    "tadmm_orth_workspace_bytes": (C.c_int, [C.c_int, C.POINTER(OrthDesc), C.POINTER(C.c_size_t)]),
    "tadmm_orth_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(OrthDesc), C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.POINTER(C.c_void_p)]),
    "tadmm_orth_l2": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tadmm_orth_plan_destroy": (C.c_int, [C.c_void_p]),
    "tadmm_stiefel_desc_bytes": (C.c_int, []),
    "tadmm_stiefel_workspace_bytes": (C.c_int, [C.c_int, C.POINTER(StiefelDesc), C.POINTER(C.c_size_t)]),
    "tadmm_stiefel_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(StiefelDesc), C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.POINTER(C.c_void_p)]),
    "tadmm_stiefel_step": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "tadmm_stiefel_adam_step": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tadmm_stiefel_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tadmm_stiefel_plan_destroy": (C.c_int, [C.c_void_p]),
    "tadmm_bertadam_desc_bytes": (C.c_int, []),
    "tadmm_bertadam_chunk": (C.c_int, []),
    "tadmm_bertadam_workspace_bytes": (C.c_int, [C.c_int, C.POINTER(BertAdamDesc), C.POINTER(C.c_size_t)]),
    "tadmm_bertadam_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BertAdamDesc), C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.POINTER(C.c_void_p)]),
    "tadmm_bertadam_step": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_void_p]),
    "tadmm_bertadam_norms": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "tadmm_bertadam_plan_destroy": (C.c_int, [C.c_void_p]),
    "tadmm_gemm_pack_bytes": (C.c_size_t, [C.c_int, C.POINTER(GemmDesc)]),
    "tadmm_gemm_pack": (C.c_int, [C.c_int, C.POINTER(GemmDesc), C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "tadmm_gemm_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tadmm_gemm": (C.c_int, [C.c_void_p, C.POINTER(GemmDesc), C.c_void_p]),
    "tadmm_gemm_bf16_nt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "tadmm_chain_desc_bytes": (C.c_int, []),
    "tadmm_conv_chain_desc_bytes": (C.c_int, []),
    "tadmm_ttconv_fused": (C.c_int, [C.c_void_p, C.POINTER(ConvChainDesc), C.c_void_p]),
    "tadmm_ttconv_fused_save": (C.c_int, [C.c_void_p, C.POINTER(ConvChainDesc), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "tadmm_ttconv_fused_bwd": (C.c_int, [C.c_void_p, C.POINTER(ConvChainDesc), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "tadmm_ttconv_fused_plan": (C.c_int, [C.POINTER(ConvChainDesc), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "tadmm_ttlinear_fwd": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_ttlinear_bwd": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_ttconv_chain_in": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_ttconv_chain_out": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_tucker_1x1": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_svdconv_fwd": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_svdconv_bwd": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_void_p]),
    "tadmm_ttlinear_fwd_save": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "tadmm_ttlinear_bwd_save": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "tadmm_svdconv_fwd_save": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "tadmm_svdconv_bwd_save": (C.c_int, [C.c_void_p, C.POINTER(ChainDesc), C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "tadmm_wgrad_desc_bytes": (C.c_int, []),
    "tadmm_wgrad_workspace_bytes": (C.c_int, [C.POINTER(WgradDesc), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "tadmm_wgrad": (C.c_int, [C.c_void_p, C.POINTER(WgradDesc), C.c_void_p, C.c_size_t, C.c_void_p]),
    "tadmm_ttm_desc_bytes": (C.c_int, []),
    "tadmm_ttm_gather_fits": (C.c_int, [C.POINTER(TtmDesc), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "tadmm_ttm_gather_fwd": (C.c_int, [C.c_void_p, C.POINTER(TtmDesc), C.c_void_p]),
    "tadmm_ttm_gather_bwd": (C.c_int, [C.c_void_p, C.POINTER(TtmDesc), C.c_void_p]),
    "tadmm_lstm_desc_bytes": (C.c_int, []),
    "tadmm_lstm_fits": (C.c_int, [C.POINTER(LstmDesc), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "tadmm_lstm_seq_fwd": (C.c_int, [C.c_void_p, C.POINTER(LstmDesc), C.c_void_p]),
    "tadmm_lstm_seq_fwd_save": (C.c_int, [C.c_void_p, C.POINTER(LstmDesc), C.c_void_p]),
    "tadmm_lstm_seq_bwd": (C.c_int, [C.c_void_p, C.POINTER(LstmDesc), C.c_void_p]),
    "tadmm_distill_desc_bytes": (C.c_int, []),
    "tadmm_distill_workspace_bytes": (C.c_int, [C.POINTER(DistillDesc), C.POINTER(C.c_size_t)]),
    "tadmm_distill_loss": (C.c_int, [C.c_void_p, C.POINTER(DistillDesc), C.c_void_p]),
    "tadmm_layer_mse_desc_bytes": (C.c_int, []),
    "tadmm_layer_mse_max_pairs": (C.c_int, []),
    "tadmm_layer_mse_geometry": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tadmm_layer_mse_workspace_bytes": (C.c_int, [C.POINTER(LayerMseDesc), C.POINTER(C.c_size_t)]),
    "tadmm_layer_mse": (C.c_int, [C.c_void_p, C.POINTER(LayerMseDesc), C.c_void_p]),
    "tadmm_attn_desc_bytes": (C.c_int, []),
    "tadmm_attn_fits": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(C.c_size_t)]),
    "tadmm_attn_workspace_bytes": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(C.c_size_t)]),
    "tadmm_attn_fwd": (C.c_int, [C.c_void_p, C.POINTER(AttnDesc), C.c_void_p]),
    "tadmm_attn_bwd": (C.c_int, [C.c_void_p, C.POINTER(AttnDesc), C.c_void_p]),
    "tadmm_bertnorm_desc_bytes": (C.c_int, []),
    "tadmm_bertnorm_fits": (C.c_int, [C.POINTER(BertNormDesc), C.POINTER(C.c_int)]),
    "tadmm_bertnorm_workspace_bytes": (C.c_int, [C.POINTER(BertNormDesc), C.POINTER(C.c_size_t)]),
    "tadmm_bertnorm_fwd": (C.c_int, [C.c_void_p, C.POINTER(BertNormDesc), C.c_void_p]),
    "tadmm_bertnorm_bwd": (C.c_int, [C.c_void_p, C.POINTER(BertNormDesc), C.c_void_p]),
    "tadmm_prenorm_desc_bytes": (C.c_int, []),
    "tadmm_prenorm_fits": (C.c_int, [C.POINTER(PreNormDesc), C.POINTER(C.c_int)]),
    "tadmm_prenorm_workspace_bytes": (C.c_int, [C.POINTER(PreNormDesc), C.POINTER(C.c_size_t)]),
    "tadmm_prenorm_fwd": (C.c_int, [C.c_void_p, C.POINTER(PreNormDesc), C.c_void_p]),
    "tadmm_prenorm_bwd": (C.c_int, [C.c_void_p, C.POINTER(PreNormDesc), C.c_void_p]),
    "tadmm_bnact_desc_bytes": (C.c_int, []),
    "tadmm_bnact_fits": (C.c_int, [C.POINTER(BnActDesc), C.POINTER(C.c_int64)]),
    "tadmm_bnact_workspace_bytes": (C.c_int, [C.POINTER(BnActDesc), C.POINTER(C.c_size_t)]),
    "tadmm_bnact_plan": (C.c_int, [C.POINTER(BnActDesc), C.POINTER(C.c_int32)]),
    "tadmm_bnact_fwd": (C.c_int, [C.c_void_p, C.POINTER(BnActDesc), C.c_void_p]),
    "tadmm_bnact_bwd": (C.c_int, [C.c_void_p, C.POINTER(BnActDesc), C.c_void_p]),
    "tadmm_densebn_desc_bytes": (C.c_int, []),
    "tadmm_densebn_max_segments": (C.c_int, []),
    "tadmm_densebn_fits": (C.c_int, [C.POINTER(DenseBnDesc), C.POINTER(C.c_int64)]),
    "tadmm_densebn_workspace_bytes": (C.c_int, [C.POINTER(DenseBnDesc), C.POINTER(C.c_size_t)]),
    "tadmm_densebn_plan": (C.c_int, [C.POINTER(DenseBnDesc), C.POINTER(C.c_int32)]),
    "tadmm_densebn_stats": (C.c_int, [C.c_void_p, C.POINTER(DenseBnDesc), C.c_void_p]),
    "tadmm_densebn_fwd": (C.c_int, [C.c_void_p, C.POINTER(DenseBnDesc), C.c_void_p]),
    "tadmm_densebn_bwd": (C.c_int, [C.c_void_p, C.POINTER(DenseBnDesc), C.c_void_p]),
    "tadmm_dwbn_desc_bytes": (C.c_int, []),
    "tadmm_dwbn_fits": (C.c_int, [C.POINTER(DwBnDesc), C.POINTER(C.c_int32)]),
    "tadmm_dwbn_plan": (C.c_int, [C.POINTER(DwBnDesc), C.POINTER(C.c_int32)]),
    "tadmm_dwbn_workspace_bytes": (C.c_int, [C.POINTER(DwBnDesc), C.POINTER(C.c_size_t)]),
    "tadmm_dwbn_fwd": (C.c_int, [C.c_void_p, C.POINTER(DwBnDesc), C.c_void_p]),
    "tadmm_dwbn_bwd": (C.c_int, [C.c_void_p, C.POINTER(DwBnDesc), C.c_void_p]),
    "tadmm_core_conv_desc_bytes": (C.c_int, []),
    "tadmm_core_conv_fwd": (C.c_int, [C.c_void_p, C.POINTER(CoreConvDesc), C.c_void_p]),
    "tadmm_core_conv_dgrad": (C.c_int, [C.c_void_p, C.POINTER(CoreConvDesc), C.c_void_p]),
    "tadmm_core_conv_wgrad_workspace_bytes": (C.c_int, [C.POINTER(CoreConvDesc), C.POINTER(C.c_size_t),
                                                        C.POINTER(C.c_int)]),
    "tadmm_core_conv_wgrad": (C.c_int, [C.c_void_p, C.POINTER(CoreConvDesc), C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "tadmm_gram_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "tadmm_gram_ld": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "tadmm_gram_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    "tadmm_eigh_scratch_bytes": (C.c_size_t, [C.c_int]),
    "tadmm_eigh_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.POINTER(C.c_int), C.c_void_p]),
    "tadmm_eigh_partial_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.POINTER(C.c_int), C.c_void_p]),
    "tadmm_dgemm_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "tadmm_dgemm3_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "tadmm_dgemm3_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tadmm_dgemm_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tadmm_dgemm_tile_prob_bytes": (C.c_int, []),
    "tadmm_dgemm_tile_check": (C.c_int, [C.c_int, C.POINTER(DgemmTileProb), C.c_int, C.c_int, C.c_int]),
    "tadmm_dgemm_tile_scratch_bytes": (C.c_size_t, [C.c_int, C.POINTER(DgemmTileProb)]),
    "tadmm_dgemm_tile_f64": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(DgemmTileProb), C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "tadmm_tile_map": (C.c_int64, [C.c_int, C.POINTER(TileMapProb), C.POINTER(C.c_int32), C.c_int64,
                                   C.POINTER(C.c_double)]),
    "tadmm_cholqr_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "tadmm_cholqr_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_int), C.c_void_p]),
}

_lib = None
_lock = threading.Lock()


def library_path():
    # TADMM_LIB: file name of an instrumented build of the same sources next to the product library (e.g. the
    # -DTADMM_TRI_STAMPS variant scripts/stamp_tri.py uses); never a fallback -- a missing file still raises
    return os.path.join(_HERE, os.path.basename(os.environ.get("TADMM_LIB", _LIB_NAME)))


def load():
    """dlopen the HIP library and bind every symbol of the ABI table.  Raises loudly."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # PyTorch-ROCm ships its own libamdhip64; import it FIRST so that this library's HIP calls resolve to the
        # same runtime instance that owns torch's device memory and streams (loading the system runtime first
        # leaves the process with a runtime torch then cannot see a device through)
        import torch  # noqa: F401
        path = library_path()
        if not os.path.exists(path):
            raise TadmmLibraryError(
                f"{path} not found: build it with `make -C dnn-compression-tensor-admm_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        try:
            lib = C.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise TadmmLibraryError(f"cannot load {path}: {e}") from e
        missing = []
        for name, (res, args) in ABI.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        if missing:
            raise TadmmLibraryError(f"{path} does not export: {', '.join(missing)}")
        a, b = C.c_int(), C.c_int()
        lib.tadmm_abi_sizes(C.byref(a), C.byref(b))
        if (a.value, b.value) != (C.sizeof(LayerDesc), C.sizeof(GemmDesc)):
            raise TadmmLibraryError(f"{path}: struct layout mismatch (library {a.value}/{b.value} bytes, "
                                    f"binding {C.sizeof(LayerDesc)}/{C.sizeof(GemmDesc)})")
        if lib.tadmm_chain_desc_bytes() != C.sizeof(ChainDesc):
            raise TadmmLibraryError(f"{path}: tadmm_chain_desc layout mismatch (library {lib.tadmm_chain_desc_bytes()} "
                                    f"bytes, binding {C.sizeof(ChainDesc)})")
        if lib.tadmm_conv_chain_desc_bytes() != C.sizeof(ConvChainDesc):
            raise TadmmLibraryError(f"{path}: tadmm_conv_chain_desc layout mismatch")
        if lib.tadmm_orth_desc_bytes() != C.sizeof(OrthDesc):
            raise TadmmLibraryError(f"{path}: tadmm_orth_desc layout mismatch")
        if lib.tadmm_stiefel_desc_bytes() != C.sizeof(StiefelDesc):
            raise TadmmLibraryError(f"{path}: tadmm_stiefel_desc layout mismatch")
        if lib.tadmm_bertadam_desc_bytes() != C.sizeof(BertAdamDesc):
            raise TadmmLibraryError(f"{path}: tadmm_bertadam_desc layout mismatch")
        if lib.tadmm_bertadam_chunk() != BERTADAM_CHUNK:
            raise TadmmLibraryError(f"{path}: tadmm_bertadam_chunk() = {lib.tadmm_bertadam_chunk()}, binding "
                                    f"{BERTADAM_CHUNK}")
        if lib.tadmm_wgrad_desc_bytes() != C.sizeof(WgradDesc):
            raise TadmmLibraryError(f"{path}: tadmm_wgrad_desc layout mismatch")
        if lib.tadmm_ttm_desc_bytes() != C.sizeof(TtmDesc):
            raise TadmmLibraryError(f"{path}: tadmm_ttm_desc layout mismatch")
        if lib.tadmm_lstm_desc_bytes() != C.sizeof(LstmDesc):
            raise TadmmLibraryError(f"{path}: tadmm_lstm_desc layout mismatch")
        if lib.tadmm_distill_desc_bytes() != C.sizeof(DistillDesc):
            raise TadmmLibraryError(f"{path}: tadmm_distill_desc layout mismatch")
        if lib.tadmm_layer_mse_desc_bytes() != C.sizeof(LayerMseDesc):
            raise TadmmLibraryError(f"{path}: tadmm_layer_mse_desc layout mismatch")
        if lib.tadmm_layer_mse_max_pairs() != LAYER_MSE_MAX_PAIRS:
            raise TadmmLibraryError(f"{path}: tadmm_layer_mse_max_pairs() = {lib.tadmm_layer_mse_max_pairs()}, binding "
                                    f"{LAYER_MSE_MAX_PAIRS}")
        if lib.tadmm_attn_desc_bytes() != C.sizeof(AttnDesc):
            raise TadmmLibraryError(f"{path}: tadmm_attn_desc layout mismatch")
        if lib.tadmm_bertnorm_desc_bytes() != C.sizeof(BertNormDesc):
            raise TadmmLibraryError(f"{path}: tadmm_bertnorm_desc layout mismatch")
        if lib.tadmm_prenorm_desc_bytes() != C.sizeof(PreNormDesc):
            raise TadmmLibraryError(f"{path}: tadmm_prenorm_desc layout mismatch")
        if lib.tadmm_bnact_desc_bytes() != C.sizeof(BnActDesc):
            raise TadmmLibraryError(f"{path}: tadmm_bnact_desc layout mismatch")
        if lib.tadmm_densebn_desc_bytes() != C.sizeof(DenseBnDesc) \
                or lib.tadmm_densebn_max_segments() != DENSEBN_MAX_SEGMENTS:
            raise TadmmLibraryError(f"{path}: tadmm_densebn_desc layout mismatch")
        if lib.tadmm_dwbn_desc_bytes() != C.sizeof(DwBnDesc):
            raise TadmmLibraryError(f"{path}: tadmm_dwbn_desc layout mismatch")
        if lib.tadmm_core_conv_desc_bytes() != C.sizeof(CoreConvDesc):
            raise TadmmLibraryError(f"{path}: tadmm_core_conv_desc layout mismatch")
        if lib.tadmm_dgemm_tile_prob_bytes() != C.sizeof(DgemmTileProb):
            raise TadmmLibraryError(f"{path}: tadmm_dgemm_tile_prob layout mismatch")
        _lib = lib
        return lib


class Handle:
    """One tadmm handle per device (not thread-safe, like the C object)."""

    _cache = {}

    def __init__(self, device_index: int):
        self.lib = load()
        self.ptr = C.c_void_p()
        rc = self.lib.tadmm_create(int(device_index), C.byref(self.ptr))
        if rc != 0:
            msg = self.lib.tadmm_last_error(self.ptr).decode() if self.ptr else "create failed"
            raise TadmmError(rc, msg)
        self.device_index = device_index

    @classmethod
    def get(cls, device_index: int) -> "Handle":
        h = cls._cache.get(device_index)
        if h is None:
            h = cls(device_index)
            cls._cache[device_index] = h
        return h

    def check(self, rc):
        if rc < 0:
            raise TadmmError(rc, self.lib.tadmm_last_error(self.ptr).decode())
        return rc


def make_layer_desc(kind, dims, tt_shapes=None, ranks=None, flags=0, hooi_max_iter=100, hooi_tol=1e-4):
    d = LayerDesc()
    d.kind = kind
    d.ndim = len(dims)
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    if kind == KIND_SVD:
        d.d = 2
        d.ranks[0] = int(ranks if isinstance(ranks, int) else ranks[0])
    elif kind == KIND_TUCKER2:
        d.d = 2
        d.ranks[0], d.ranks[1] = int(ranks[0]), int(ranks[1])
    else:
        if len(tt_shapes) > MAX_MODES:
            raise ValueError(f"at most {MAX_MODES} TT modes are supported")
        d.d = len(tt_shapes)
        for i, v in enumerate(tt_shapes):
            d.tt_shapes[i] = int(v)
        if len(ranks) != len(tt_shapes) + 1:
            raise ValueError("len(ranks) must be len(tt_shapes)+1")
        for i, v in enumerate(ranks):
            d.ranks[i] = int(v)
    d.flags = flags
    d.hooi_max_iter = hooi_max_iter
    d.hooi_tol = hooi_tol
    return d


def clamp_ranks(tt_shapes, ranks):
    """ttd.py:18-19 -- the rank clamp as a pure function of shapes (host only)."""
    lib = load()
    dims = [1, 1]
    d = LayerDesc()
    d.kind = KIND_TT_LINEAR
    d.ndim = 2
    d.dims[0], d.dims[1] = dims
    d.d = len(tt_shapes)
    for i, v in enumerate(tt_shapes):
        d.tt_shapes[i] = int(v)
    for i, v in enumerate(ranks):
        d.ranks[i] = int(v)
    rc = lib.tadmm_tt_clamp_ranks(C.byref(d))
    if rc < 0:
        raise TadmmError(rc, "tadmm_tt_clamp_ranks: invalid descriptor")
    return [int(d.ranks[i]) for i in range(len(ranks))]
