"""ctypes binding of libgsv_hip.so (include/gsv.h).  The product path has no CPU or
PyTorch fallback: if the library cannot be loaded, or a call fails, this raises."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgsv_hip.so")

GSV_F32, GSV_F16 = 0, 1
GSV_OUT_S16, GSV_OUT_MULAW, GSV_OUT_ALAW, GSV_OUT_F32 = 0, 1, 2, 3   # out_fmt of gsv_postprocess_groups_rate


class T2SConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_layer", "dim", "n_head", "ffn_dim", "vocab", "phoneme_vocab", "bert_dim")]


class SamplingParams(C.Structure):
    _fields_ = [("top_k", C.c_int), ("top_p", C.c_float), ("temperature", C.c_float),
                ("repetition_penalty", C.c_float), ("early_stop_num", C.c_int), ("eos_mask_steps", C.c_int),
                ("max_steps", C.c_int), ("seed", C.c_uint64)]


class RowSampling(C.Structure):
    """gsv_row_sampling_t: the sampling parameters of one batch row"""
    _fields_ = [("top_k", C.c_int), ("top_p", C.c_float), ("temperature", C.c_float), ("repetition_penalty", C.c_float)]


class RowLimits(C.Structure):
    """gsv_row_limits_t: the EOS horizon, early stop and step budget of one batch row"""
    _fields_ = [("eos_mask_steps", C.c_int), ("early_stop_num", C.c_int), ("max_steps", C.c_int), ("reserved", C.c_int)]


class LoudSpan(C.Structure):
    """gsv_loud_span: sentences [first, first + count) of one group, metered together; target NaN = meter only"""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("gaps", C.c_int32), ("target", C.c_float), ("peak_db", C.c_float)]


class AlignSpan(C.Structure):
    """gsv_align_span_t: frame rows [f0, f0 + nf) x phoneme rows [l0, l0 + nl) of one alignment; ends go to ends[out0:out0 + nl]"""
    _fields_ = [(n, C.c_int32) for n in ("f0", "nf", "l0", "nl", "out0", "reserved")]


class AlignSegSpan(C.Structure):
    """gsv_align_seg_span_t: codes [code0, code0 + n_codes) and phones [phone0, phone0 + n_phones) of one segment of a decode"""
    _fields_ = [(n, C.c_int32) for n in ("segment", "code0", "n_codes", "phone0", "n_phones")]


ALIGN_SPAN_DTYPE = [(n, "<i4") for n in ("f0", "nf", "l0", "nl", "out0", "reserved")]   # numpy view of a span table

LOUD_LIMITED, LOUD_NAN, LOUD_SILENT = 1, 2, 4   # gsv_loud_report.flags
LOUD_REPORT_DTYPE = [("lufs", "<f8"), ("gain", "<f4"), ("flags", "<u4")]   # numpy view of gsv_loud_report [n_spans]


class VitsConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("inter_channels", "hidden_channels", "filter_channels", "n_heads", "n_layers",
                                        "kernel_size", "gin_channels", "n_symbols", "ssl_dim", "n_bins",
                                        "upsample_initial_channel", "n_ups")] + \
               [("up_rates", C.c_int * 8), ("up_kernels", C.c_int * 8), ("n_resblocks", C.c_int),
                ("rb_kernels", C.c_int * 4), ("rb_dilations", (C.c_int * 3) * 4), ("ref_bins", C.c_int),
                ("flavor", C.c_int), ("v2pro", C.c_int)]


class VocoderConfig(C.Structure):
    _fields_ = [("kind", C.c_int), ("in_channels", C.c_int), ("upsample_initial_channel", C.c_int), ("n_ups", C.c_int),
                ("up_rates", C.c_int * 8), ("up_kernels", C.c_int * 8), ("n_resblocks", C.c_int),
                ("rb_kernels", C.c_int * 4), ("rb_dilations", (C.c_int * 3) * 4), ("bias_at_final", C.c_int),
                ("tanh_at_final", C.c_int), ("snake_logscale", C.c_int)]


class DitConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dim", "depth", "heads", "dim_head", "ff_mult", "mel_dim", "text_dim", "conv_layers")]


class BweConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_fft", "hop_size", "win_size", "channels", "layers", "hr_sampling_rate")]


class ConvDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("res", C.c_void_p),
                ("T_in", C.c_int), ("T_out", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("taps", C.c_int),
                ("stride", C.c_int), ("dil", C.c_int), ("pad", C.c_int), ("pre_act", C.c_int),
                ("pre_slope", C.c_float), ("post_act", C.c_int), ("scale", C.c_float), ("accumulate", C.c_int),
                ("out_f32", C.c_int), ("ups_u", C.c_int), ("ups_pad", C.c_int),
                ("Z", C.c_int), ("xz", C.c_longlong), ("wz", C.c_longlong), ("yz", C.c_longlong),
                ("ldx", C.c_int), ("ldw", C.c_int), ("ldy", C.c_int), ("gate", C.c_void_p), ("bz", C.c_int),
                ("rz", C.c_longlong), ("ldr", C.c_int),
                # optional, 0 = default: residual dtype (0 follows out_f32, 1 fp32, 2 engine dtype), slice column offset in y,
                # non-temporal weights, batched residual slices (include/gsv.h)
                ("res_dtype", C.c_int), ("y_col0", C.c_int), ("w_nt", C.c_int), ("z_res", C.c_int),
                # optional, 0 = one gate vector: per-row gates (output row t takes gate + (t / gate_rows) * gate_ld)
                ("gate_rows", C.c_int), ("gate_ld", C.c_int)]


class ZeroMaps(C.Structure):
    """gsv_zero_maps: the base pointers of the maps one gsv_op_zero_rows launch covers"""
    _fields_ = [("p", C.c_void_p * 8)]


_SIGS = {
    "gsv_init": (C.c_int, [C.c_int]),
    "gsv_last_error": (C.c_char_p, []),
    "gsv_abi_version": (C.c_int, []),
    "gsv_t2s_create": (C.c_int, [C.POINTER(T2SConfig), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "gsv_t2s_destroy": (None, [C.c_void_p]),
    "gsv_t2s_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "gsv_t2s_finalize": (C.c_int, [C.c_void_p]),
    "gsv_t2s_prefill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p]),
    "gsv_t2s_prefill_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "gsv_t2s_set_row_rng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gsv_t2s_set_row_sampling": (C.c_int, [C.c_void_p, C.POINTER(RowSampling), C.c_int]),
    "gsv_t2s_set_row_limits": (C.c_int, [C.c_void_p, C.POINTER(RowLimits), C.c_int]),
    "gsv_t2s_decode": (C.c_int, [C.c_void_p, C.POINTER(SamplingParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_int), C.c_void_p]),
    "gsv_t2s_session_begin": (C.c_int, [C.c_void_p, C.POINTER(SamplingParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_t2s_session_admit": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_t2s_session_advance": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_t2s_session_release": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_t2s_session_end": (C.c_int, [C.c_void_p]),
    "gsv_t2s_session_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gsv_t2s_session_adopt_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "gsv_t2s_decode_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "gsv_t2s_set_mega": (C.c_int, [C.c_void_p, C.c_int]),
    "gsv_t2s_set_prefill_gemm": (C.c_int, [C.c_void_p, C.c_int]),
    "gsv_t2s_debug_kv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gsv_t2s_engine_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]),
    "gsv_t2s_set_debug": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_t2s_set_logprobs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gsv_t2s_debug_stall": (C.c_int, [C.c_void_p, C.c_int]),
    "gsv_t2s_debug_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_t2s_time_step": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]),
    "gsv_t2s_debug_set_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gsv_t2s_step_bytes": (C.c_int64, [C.c_void_p, C.POINTER(C.c_int64)]),
    "gsv_vits_create": (C.c_int, [C.POINTER(VitsConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "gsv_vits_destroy": (None, [C.c_void_p]),
    "gsv_vits_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "gsv_vits_finalize": (C.c_int, [C.c_void_p]),
    "gsv_vits_set_refer": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                                     C.c_void_p]),
    "gsv_vits_set_refer_sv": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p),
                                        C.c_int, C.c_void_p]),
    "gsv_vits_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                  C.c_double, C.c_uint64, C.c_void_p, C.c_void_p]),
    "gsv_vits_encp_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "gsv_vits_decode_encp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "gsv_vits_extract_latent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_vits_debug_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                        C.c_void_p]),
    "gsv_vits_set_align": (C.c_int, [C.c_void_p, C.POINTER(AlignSegSpan), C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_vits_last_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gsv_vits_store_voice": (C.c_int, [C.c_void_p, C.c_int]),
    "gsv_vits_decode_segments": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_void_p, C.c_float, C.c_void_p,
                                           C.c_void_p]),
    "gsv_vits_decode_segments_speed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int),
                                                 C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_void_p,
                                                 C.c_float, C.c_void_p, C.c_void_p]),
    "gsv_vits_segment_gap": (C.c_int, [C.POINTER(VitsConfig)]),
    "gsv_vits_segment_map": (C.c_int, [C.POINTER(VitsConfig), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                       C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]),
    "gsv_vits_segment_map_speed": (C.c_int, [C.POINTER(VitsConfig), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]),
    "gsv_vocoder_create": (C.c_int, [C.POINTER(VocoderConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "gsv_vocoder_destroy": (None, [C.c_void_p]),
    "gsv_vocoder_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "gsv_vocoder_finalize": (C.c_int, [C.c_void_p]),
    "gsv_vocoder_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_vocoder_forward_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "gsv_vocoder_segment_gap": (C.c_int, [C.POINTER(VocoderConfig)]),
    "gsv_vocoder_segment_map": (C.c_int, [C.POINTER(VocoderConfig), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int32),
                                          C.c_int64]),
    "gsv_cfm_create": (C.c_int, [C.POINTER(DitConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "gsv_cfm_destroy": (None, [C.c_void_p]),
    "gsv_cfm_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "gsv_cfm_finalize": (C.c_int, [C.c_void_p]),
    "gsv_cfm_inference": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]),
    "gsv_cfm_inference_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_float, C.c_void_p, C.c_void_p]),
    "gsv_cfm_inference_guided": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_float, C.c_float, C.c_void_p,
                                           C.c_void_p]),
    "gsv_cfm_adapter_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "gsv_cfm_adapter_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "gsv_cfm_adapter_finalize": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "gsv_cfm_adapter_remove": (C.c_int, [C.c_void_p, C.c_int]),
    "gsv_cfm_adapter_count": (C.c_int, [C.c_void_p]),
    "gsv_cfm_inference_adapted": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_float, C.c_float,
                                            C.c_void_p, C.c_void_p]),
    "gsv_cfm_session_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "gsv_cfm_session_admit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_uint64),
                                        C.c_void_p]),
    "gsv_cfm_session_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "gsv_cfm_session_fetch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_cfm_session_fetch_mel": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.c_longlong, C.c_float,
                                            C.c_float, C.c_void_p, C.c_void_p]),
    "gsv_cfm_session_release": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "gsv_cfm_session_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "gsv_cfm_session_end": (C.c_int, [C.c_void_p]),
    "gsv_sola": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "gsv_postprocess": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_postprocess_f32": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "gsv_postprocess_groups_workspace": (C.c_longlong, [C.POINTER(C.c_int), C.c_int]),
    "gsv_postprocess_groups": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "gsv_postprocess_groups_rate_workspace": (C.c_longlong, [C.POINTER(C.c_int), C.c_int, C.c_int]),
    "gsv_postprocess_groups_rate": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gsv_postprocess_groups_loud_workspace": (C.c_longlong, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                             C.c_int, C.c_int, C.c_int]),
    "gsv_postprocess_groups_loud": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(LoudSpan), C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_op_loudness": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.c_int, C.c_int, C.POINTER(LoudSpan), C.c_int, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_bwe_create": (C.c_int, [C.POINTER(BweConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "gsv_bwe_destroy": (None, [C.c_void_p]),
    "gsv_bwe_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "gsv_bwe_finalize": (C.c_int, [C.c_void_p]),
    "gsv_bwe_out_len": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gsv_bwe_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_bwe_debug_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "gsv_aa_act_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gsv_op_flash_attn64": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_op_flash_attn64_seg": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "gsv_op_flash_attn64_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "gsv_op_flash_attn64_seg_qt": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_float, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "gsv_op_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p,
                                   C.c_int, C.c_void_p]),
    "gsv_debug_last_attn_route": (C.c_uint64, [C.c_int]),
    "gsv_op_embed_ln": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "gsv_op_flash_rel96": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "gsv_op_conv1d": (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_void_p]),
    "gsv_op_gemm_panel": (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_int, C.c_void_p]),
    "gsv_debug_last_conv_route": (C.c_uint64, [C.c_int]),
    "gsv_debug_last_pair_route": (C.c_uint64, [C.c_int]),
    "gsv_op_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "gsv_op_magnitude": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_op_conv_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "gsv_op_conv_pair_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_op_aa_act_cl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gsv_op_aff_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "gsv_op_time_mean": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_op_channel_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p]),
    "gsv_op_channel_norm_seg": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                          C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gsv_op_gather_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "gsv_op_zero_rows": (C.c_int, [C.POINTER(ZeroMaps), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "gsv_op_time_mean_seg": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                       C.c_void_p]),
    "gsv_op_resample_poly_seg": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_op_frame_seg": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p]),
    "gsv_op_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_float, C.c_int, C.c_void_p]),
    "gsv_op_lora_delta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p]),
    "gsv_op_decode_attn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p]),
    "gsv_op_prefill_attn": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_op_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                C.POINTER(SamplingParams), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_op_sample_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(RowSampling),
                                     C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_op_token_logprob": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_op_align_workspace": (C.c_longlong, [C.c_int, C.POINTER(AlignSpan), C.POINTER(C.c_int64)]),
    "gsv_op_align_logp": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "gsv_op_align_path": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsv_op_align": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                               C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
}

EXPORTS = tuple(_SIGS)   # every symbol include/gsv.h declares
VITS_MAX_VOICES = 128    # GSV_VITS_MAX_VOICES (gsv.h): voice slots of the segmented decode
CFM_MAX_ADAPTERS = 256   # GSV_CFM_MAX_ADAPTERS (gsv.h): LoRA adapters one DiT engine holds at once
LORA_MAX_RANK = 128      # GSV_LORA_MAX_RANK (gsv.h)
CFM_SESSION_MAX_ROWS = 64   # GSV_CFM_SESSION_MAX_ROWS (gsv.h): slots / live DiT rows of one flow-matching session

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python gpt-sovits_amd/gsv/build.py` "
                               "(the gsv hot path has no CPU fallback)")
        # torch first: it ships its own HIP runtime; loading ours before it puts two runtimes in one
        # process and the second one finds no device
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(l, name)
            except AttributeError:   # tests/test_abi.py asserts the full export list
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().gsv_last_error().decode(errors="replace")
        raise RuntimeError(f"libgsv_hip {what} failed (rc={rc}): {msg}")


def load_tensors(fn, handle, items):
    """stages every (name, tensor) of `items` in an engine handle through its gsv_*_load_tensor `fn`, as fp32 host copies"""
    import torch
    for k, v in items:
        t = v.detach().to("cpu", torch.float32).contiguous()
        check(fn(handle, k.encode(), t.data_ptr(), t.numel()), f"load {k}")


_inited = set()


def init(device_index: int):
    if device_index not in _inited:
        check(lib().gsv_init(device_index), "gsv_init")
        _inited.add(device_index)


def dtype_code(torch_dtype) -> int:
    import torch
    if torch_dtype == torch.float16:
        return GSV_F16
    if torch_dtype == torch.float32:
        return GSV_F32
    raise ValueError(f"unsupported dtype {torch_dtype}: the engine computes in float16 or float32")
