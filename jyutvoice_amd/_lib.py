"""ctypes binding of libjyutvoice_hip.so (include/jyutvoice_hip.h).

The library is the product; there is no Python/CPU fallback.  `load()` raises if the shared object is
missing or cannot be loaded, and every wrapper raises `JvError` with the library's own message when a
call fails.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JYUTVOICE_HIP_LIB") or os.path.join(HERE, "libjyutvoice_hip.so")

JV_MODEL_TTS = 0
JV_MODEL_HIFT = 1
JV_MODEL_PROMPT = 2
JV_MODEL_FLOW = 3      # the decoder.* / spk_embed_affine_layer.* part of JV_MODEL_TTS (jv_finalize only)

JV_PRECISION_FP32 = 0
JV_PRECISION_FP16 = 1     # jv_flow_set_precision: the estimator's fp16x3 contractions issue the hi x hi product alone

SOLVERS = {"euler": 0, "midpoint": 1, "heun": 2}      # jv_flow_set_solver: JV_SOLVER_EULER / _MIDPOINT / _HEUN
# jv_cfm_pool_step_s: JV_STAGE_* -- bit 0 saves x0, bit 1 saves k1, bit 2 starts from x0, bit 3 adds k1
STAGE_EULER, STAGE_MID1, STAGE_MID2, STAGE_HEUN1, STAGE_HEUN2 = 0, 1, 4, 3, 12

JV_ENC_ATTN_AUTO = 0    # jv_encoder_set_attention: four launches up to 512 tokens, encattn.hip's one launch above
JV_ENC_ATTN_FUSED = 1
JV_ENC_ATTN_GEMM = 2

# jv_hift_decode_tap: tap name -> (id, channels, positions per mel frame, + positions) as include/jyutvoice_hip.h lists them
HIFT_TAPS = {"STFT": (0, 18, 120, 1), "PRE": (1, 512, 1, 0), "POST": (14, 18, 120, 1), "FRAMES": (15, 16, 120, 1)}
for _i_lvl, (_c, _m, _a) in enumerate(((256, 8, 0), (128, 40, 0), (64, 120, 1))):
    for _k, _name in enumerate(("UP", "SI", "XS", "X")):
        HIFT_TAPS[f"{_name}{_i_lvl}"] = (2 + 3 * _k + _i_lvl, _c, _m, _a)

# jv_encoder_fwd_tap: tap name -> (id, channels), in execution order, as include/jyutvoice_hip.h lists them (JV_ENC_TAP_*: the five
# taps of encoder layer i are the layer-0 ids + 5 i)
ENC_TAPS = {"EMB": (0, 192), "PRE0": (1, 192), "PRE1": (2, 192), "PRE2": (3, 192), "H0": (4, 576)}
for _i_layer in range(6):
    for _k, (_name, _c) in enumerate((("QKV", 1728), ("ATT", 576), ("N1", 576), ("FF", 768), ("N2", 576))):
        ENC_TAPS[f"{_name}{_i_layer}"] = (5 + 5 * _i_layer + _k, _c)
ENC_TAPS.update({"XD": (35, 576), "D1": (36, 256), "D2": (37, 256)})

# jv_upsample_encoder_tap: tap name -> (id, channels, rate), in execution order, as include/jyutvoice_hip.h lists them (JV_UPS_TAP_*).
# rate 1: token rows, out [B, C, P + N]; rate 2: mel rows, out [B, C, 2 (P + N)].  The eight taps of token-rate block i are NAME_i
# (block-0 id + 8 i), of mel-rate block i NAME_ui.  UPS_TABLES (PE1, PE2, POS_*): [2T - 1, 512] with T the encoded width x rate
UPS_MODES = {"prompt": 0, "flow": 1, "partial": 2, "ctx": 3}
UPS_BLOCK_TAPS = (("LN1", 512), ("QKV", 1536), ("POS", 512), ("ATT", 512), ("X1", 512), ("LN2", 512), ("FF", 2048), ("X2", 512))
UPS_TAPS = {"EMB": (0, 512, 1), "EL": (1, 512, 1), "E0": (2, 512, 1), "PE1": (3, 512, 1), "C1": (4, 512, 1), "LA": (5, 512, 1)}
for _i_blk in range(6):
    for _k, (_name, _c) in enumerate(UPS_BLOCK_TAPS):
        UPS_TAPS[f"{_name}_{_i_blk}"] = (6 + 8 * _i_blk + _k, _c, 1)
UPS_TAPS.update({"REP": (54, 512, 2), "UP": (55, 512, 2), "UL": (56, 512, 2), "U0": (57, 512, 2), "PE2": (58, 512, 2)})
for _i_blk in range(4):
    for _k, (_name, _c) in enumerate(UPS_BLOCK_TAPS):
        UPS_TAPS[f"{_name}_u{_i_blk}"] = (59 + 8 * _i_blk + _k, _c, 2)
UPS_TAPS.update({"AN": (91, 512, 2), "H": (92, 80, 2)})
UPS_TABLES = frozenset(k for k in UPS_TAPS if k.startswith(("PE", "POS_")))

# jv_flow_estimator_tap: tap name -> (id, channels), in execution order, as include/jyutvoice_hip.h lists them (JV_EST_TAP_*).  The
# time taps (EST_TIME_TAPS) are [n, C] -- n = B2 samples in the "entry" mode, 1 in the "step" mode; every other tap is [samples, C, T]
# with samples = B2 ("entry") or 2 B ("step": the B utterances, then their unconditional twins).  RESi / BLKi_j: stage i = 0 .. 13
EST_MODES = {"entry": 0, "step": 1}
EST_STAGES, EST_BLOCKS = 14, 4
EST_TAPS = {"TSIN": (0, 320), "T1": (1, 1024), "TMISH": (2, 1024), "TEMB": (3, EST_STAGES * 256), "XIN": (4, 320)}
for _i_stage in range(EST_STAGES):
    _id0 = 5 if _i_stage == 0 else 11 + 5 * (_i_stage - 1)
    EST_TAPS[f"RES{_i_stage}"] = (_id0, 256)
    for _j in range(EST_BLOCKS):
        EST_TAPS[f"BLK{_i_stage}_{_j}"] = (_id0 + 1 + _j, 256)
    if _i_stage == 0:
        EST_TAPS["DOWN"] = (10, 256)
EST_TAPS.update({"UPC": (76, 256), "FIN": (77, 256), "D": (78, 80)})
EST_TIME_TAPS = ("TSIN", "T1", "TMISH", "TEMB")

ACT = {"none": 0, "relu": 1, "gelu": 2, "mish": 3, "elu": 4, "silu": 5}
PRO = {"none": 0, "snake": 1, "lrelu": 2}


class JvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libjyutvoice_hip error {code}: {msg}")
        self.code = code
        self.msg = msg


_p = C.c_void_p
_f = C.c_float
_i = C.c_int
_i64 = C.c_int64

# name -> (restype, argtypes); must list every symbol include/jyutvoice_hip.h declares (tests/test_abi.py)
SIGNATURES = {
    "jv_create": (_i, [C.POINTER(_p), _i, _i, _i, _i]),
    "jv_destroy": (None, [_p]),
    "jv_reserve": (_i, [_p, _i, _i, _i]),
    "jv_usable": (_i, [_p]),
    "jv_last_error": (C.c_char_p, []),
    "jv_num_tensors": (_i, [_p]),
    "jv_tensor_name": (C.c_char_p, [_p, _i]),
    "jv_tensor_model": (_i, [_p, _i]),
    "jv_tensor_ndim": (_i, [_p, _i]),
    "jv_tensor_dim": (_i64, [_p, _i, _i]),
    "jv_load_tensor": (_i, [_p, C.c_char_p, _p, C.POINTER(_i64), _i, _i, _p]),
    "jv_load_noise": (_i, [_p, _p, _i64, _i, _p]),
    "jv_finalize": (_i, [_p, _i, _p]),
    "jv_flow_estimator_step": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "jv_flow_estimator_masked": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "jv_flow_estimator_tap": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _i64, _p]),
    "jv_flow_set_streaming": (_i, [_p, _i]),
    "jv_flow_set_graph": (_i, [_p, _i]),
    "jv_flow_set_guidance": (_i, [_p, _p, _i]),
    "jv_flow_set_solver": (_i, [_p, _i]),
    "jv_flow_set_contraction": (_i, [_p, _i]),
    "jv_flow_set_precision": (_i, [_p, _i]),
    "jv_flow_contraction_info": (_i, [_p, _p, _i]),
    "jv_cfm_solve": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _f, _p, _p, _p]),
    "jv_cfm_solve_prompted": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _p, _p]),
    "jv_cfm_pool_admit": (_i, [_p] * 9 + [_i] * 4 + [_p] * 5 + [_i, _i, _p]),
    "jv_cfm_pool_step": (_i, [_p] * 6 + [_i, _i] + [_p] * 4 + [_i, _p]),
    "jv_cfm_pool_step_g": (_i, [_p] * 6 + [_i, _i] + [_p] * 5 + [_i, _p]),
    "jv_cfm_pool_step_s": (_i, [_p] * 8 + [_i, _i] + [_p] * 6 + [_i, _p]),
    "jv_cfm_pool_fetch": (_i, [_p, _p, _i, _i, _p, _p, _p, _i, _i, _p, _p]),
    "jv_flow_encoder_fwd": (_i,[_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "jv_flow_token2mel": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p]),
    "jv_flow_encoder_fwd_partial": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "jv_flow_token2mel_partial": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p]),
    "jv_flow_encoder_fwd_ctx": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "jv_upsample_encoder_tap": (_i, [_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _i64, _p]),
    "jv_flow_token2mel_ctx": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p]),
    "jv_encoder_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p]),
    "jv_encoder_fwd_tap": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p, _i64, _p]),
    "jv_encoder_set_attention": (_i, [_p, _i]),
    "jv_load_mel_basis": (_i, [_p, _p, _i64, _i, _p]),
    "jv_mel_spectrogram": (_i, [_p, _p, _i, _i, _p, _p]),
    "jv_mel_spectrogram_ragged": (_i, [_p, _p, _p, _i, _i, _p, _p, _p]),
    "jv_resample_length": (_i64, [_i64, _i, _i]),
    "jv_resample_table": (_i, [_i, _i, _p, _i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "jv_resample": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _i64, _p, _p]),
    "jv_fbank_frames": (_i64, [_i64]),
    "jv_whisper_frames": (_i64, [_i64]),
    "jv_kaldi_mel_banks": (_i, [_p]),
    "jv_load_whisper_filters": (_i, [_p, _p, _i64, _i, _p]),
    "jv_fbank": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "jv_whisper_log_mel": (_i, [_p, _p, _p, _i, _i, _p, _p, _p]),
    "jv_kweight_coeffs": (_i, [_i, C.POINTER(C.c_double)]),
    "jv_loudness_blocks": (_i64, [_i64, _i]),
    "jv_trim_bounds": (_i, [_p, _p, _p, _i, _i, _f, _i, _i, _p, _p, _p]),
    "jv_peak": (_i, [_p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "jv_loudness": (_i, [_p, _p, _p, _i, _i, _i, _p, _p]),
    "jv_level_gain": (_i, [_p, _p, _p, _i, C.c_double, C.c_double, _p, _p]),
    "jv_level_apply": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _i64, _p, _p]),
    "jv_log_prior": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "jv_maximum_path": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "jv_align": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p]),
    "jv_align_losses": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "jv_cfm_loss_inputs": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "jv_masked_mse": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p]),
    "jv_prompt_encoder_fwd": (_i, [_p, _p, _p, _i, _i, _p, _p]),
    "jv_length_regulate": (_i, [_p, _p, _p, _p, _i, _i, _f, _p, _p, _i, _p, _p, _p]),
    "jv_hift_f0": (_i, [_p, _p, _p, _i, _i, _p, _p]),
    "jv_hift_source": (_i, [_p, _p, _p, _p, _i, _i, _p, _p]),
    "jv_hift_source_seeded": (_i, [_p, _p, _p, C.c_uint64, C.c_uint32, _i, _i, _p, _p]),
    "jv_hift_source_cont": (_i, [_p, _p, _p, C.c_uint64, C.c_uint32, _i64, _p, _i, _i, _p, _p]),
    "jv_hift_source_cont_rows": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "jv_slab_copy": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _p, _i, _i, _i, _p]),
    "jv_hift_decode": (_i, [_p, _p, _p, _p, _i, _i, _p, _p]),
    "jv_hift_decode_tap": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _i64, _p]),
    "jv_op_conv_gemm": (_i, [_p, _i64, _i, _i, _i, _i, _i, _p, _i, _p, _i, _i, _p, _f, _p, _p, _f, _p, _p, _p, _p]),
    "jv_op_attention": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "jv_op_rel_attention": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    "jv_op_enc_attention": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "jv_h3_scale_for_bound": (_f, [_f]),
    "jv_op_set_products": (_i, [_i]),
    "jv_op_conv_h3_measured": (_i, [_p, _i64, _i, _i, _i, _i, _i, _p, _i, _p, _i, _i, _p, _f, _p, _p, _p, _f, _p, _p, _p]),
    "jv_op_splitk": (_i, [_p, _i64, _i, _i, _i, _i, _p, _i, _p, _p, _p, _i, _p, _p, _p, _i, _p, _i64, _p, _i64, _p, _p, _p, _i, _i, _p, _f,
                          _i, _i, _i, _p, _p]),
    "jv_op_attention_h3": (_i, [_p, _p, _i, _i, _i, _i, _f, _f, _f, _p, _p]),
    "jv_op_linear_h3": (_i, [_p, _i64, _i, _i, _p, _i, _p, _i, _p, _f, _i, _p, _p]),
    "jv_op_attention_planes": (_i, [_p, _i64, _p, _i, _i, _i, _i, _f, _f, _f, _i, _f, _p, _p, _p]),
    "jv_hift_lds_bytes": (_i, [_i, _i, _i, _i, _i]),
    "jv_op_hiftconv": (_i, [_p, _i64, _i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _i, _p, _f, _i, _i, _i, _p, _p, _p, _p]),
    "jv_op_rowconv": (_i, [_p, _i64, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p]),
    "jv_op_rowgemm": (_i, [_p, _i64, _i, _i, _p, _i, _p, _i, _p, _p, _p, _f, _f, _i, _p, _p, _p, _p]),
    "jv_op_layernorm": (_i, [_p, _p, _p, _f, _i64, _i, _p, _p]),
    "jv_op_rowgemm_qkv": (_i, [_p, _p, _i64, _i, _i, _p, _f, _f, _f, _i, _i, _p, _p, _p]),
    "jv_op_rowres": (_i, [_p, _i64, _i, _i, _p, _p, _i, _i, _i, _p] + [_p] * 13 + [_f, _p, _p, _f, _f, _p, _p, _p, _p, _p]),
    "jv_op_hiftpair": (_i, [_p, _i64, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _f, _i, _p, _p, _p]),
    "jv_op_rowblock": (_i, [_p, _p, _i64, _i, _i, _i, _f, _p, _p, _p, _p, _f, _p, _p, _f, _p, _p, _p, _p, _f, _p, _f, _f, _p, _i64,
                            _p, _p, _p, _p, _p, _p, _p, _p]),
    "jv_profile_enable": (_i, [_i]),
    "jv_profile_report": (_i, [C.c_char_p, _i64]),
}

_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library (building it is `python -m jyutvoice_amd.build` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be the first HIP runtime in the process so that this
    # library binds to the same runtime instance (device pointers and streams are shared with torch).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m jyutvoice_amd.build` (needs hipcc). "
            "jyutvoice_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().jv_last_error()
        raise JvError(rc, msg.decode("utf-8", "replace") if msg else "?")
