"""ctypes binding of libpvq.so (include/pvq.h).  Fails loudly if the HIP library is missing:
there is no CPU fallback anywhere in this package."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PVQ_DEV_LIB=1 selects the developer build of the same sources (libpvq_dev.so, -DPVQ_DEV_KNOBS: it alone reads the PVQ_* environment
# knobs that the tile-shape / fallback tests, the A/B scripts and the phase-stamp tools use).  The product library reads no environment.
# PVQ_DEV_LIB=<name> (anything else) selects lib/libpvq_<name>.so: a developer build of OTHER sources kept beside it for a same-box A/B of two
# code versions (scripts/dev_ab_knob.py PVQ_DEV_LIB 1,<name>); such files are never committed or shipped.
_dev = os.environ.get("PVQ_DEV_LIB", "")
LIB_PATH = os.path.join(_HERE, "lib", "libpvq.so" if not _dev else ("libpvq_dev.so" if _dev == "1" else "libpvq_%s.so" % _dev))

# every symbol include/pvq.h declares
EXPORTS = [
    "pvq_status_string", "pvq_last_error", "pvq_abi_version", "pvq_vqt_default_params", "pvq_vqt_create",
    "pvq_vqt_destroy", "pvq_vqt_get_params", "pvq_vqt_n_bins", "pvq_vqt_delay_seconds", "pvq_vqt_window_union",
    "pvq_vqt_n_groups", "pvq_vqt_group_info", "pvq_vqt_group_csr", "pvq_vqt_filter_params",
    "pvq_vqt_calculate_instant_db", "pvq_vqt_calculate_batch_db", "pvq_vqt_calculate_batch_db_device",
    "pvq_vqt_set_algo", "pvq_vqt_last_algo", "pvq_vqt_resolve_algo", "pvq_analysis_default_params", "pvq_analyze_batch_device",
    "pvq_analyze_batch", "pvq_vqt_analyze_batch_device", "pvq_vqt_calculate_batch_db_streams", "pvq_vqt_analyze_batch_streams", "pvq_plan_shard", "pvq_vqt_analyze_batch_multi", "pvq_vqt_set_profiling", "pvq_vqt_last_kernel_ms",
    "pvq_vqt_kernel_name", "pvq_vqt_last_kernel_launches", "pvq_vqt_last_frames_per_launch", "pvq_vqt_set_gemm_precision", "pvq_vqt_set_workspace_limit", "pvq_vqt_blockdft_columns", "pvq_vqt_set_twiddle_fp16",
    "pvq_analysis_full_default_params", "pvq_analysis_state_create", "pvq_analysis_state_destroy",
    "pvq_analysis_batch_create", "pvq_analysis_batch_destroy", "pvq_analysis_batch_update_vqt_smoothing_duration",
    "pvq_analysis_batch_preprocess_device", "pvq_analysis_batch_preprocess_pcm", "pvq_analysis_batch_get_field", "pvq_analysis_batch_get_scalars",
    "pvq_analysis_state_update_vqt_smoothing_duration", "pvq_analysis_state_preprocess",
    "pvq_analysis_state_bin_to_frequency", "pvq_analysis_state_n_buckets", "pvq_analysis_state_get_field",
    "pvq_analysis_state_get_peaks", "pvq_analysis_state_get_peaks_continuous", "pvq_analysis_state_scene_calmness",
    "pvq_analysis_state_tuning_grid_inaccuracy",
    "pvq_mono_agc_create", "pvq_mono_agc_destroy", "pvq_mono_agc_freeze_gain", "pvq_mono_agc_is_gain_frozen",
    "pvq_mono_agc_gain", "pvq_mono_agc_process", "pvq_train_chunk_samples", "pvq_train_condition_stream",
    "pvq_agc_batch_create", "pvq_agc_batch_destroy", "pvq_agc_batch_condition_device", "pvq_agc_batch_get_gains",
    "pvq_train_frames_db", "pvq_train_rows", "pvq_npy_write_f32", "pvq_stream_create", "pvq_stream_destroy",
    "pvq_stream_push", "pvq_stream_gain", "pvq_stream_chunk_size_ms", "pvq_stream_frame_db", "pvq_stream_read",
    "pvq_calculate_color", "pvq_led_frame", "pvq_host_alloc", "pvq_host_free",
    "pvq_spectrogram_row", "pvq_chroma_row", "pvq_render_batch_create", "pvq_render_batch_destroy", "pvq_render_batch_rows_device",
    "pvq_scene_default_settings", "pvq_scene_state_create", "pvq_scene_state_destroy", "pvq_scene_state_n_bins", "pvq_scene_state_n_segments",
    "pvq_scene_state_update", "pvq_scene_state_get", "pvq_scene_batch_create", "pvq_scene_batch_destroy", "pvq_scene_batch_n_segments",
    "pvq_scene_batch_frames_device", "pvq_scene_batch_get_state",
    "pvq_ml_scene_state_update", "pvq_ml_midi_pitch", "pvq_ml_scene_batch_frames_device",
    "pvq_spectrum_mesh", "pvq_calmness_histogram_mesh", "pvq_calmness_graph_create", "pvq_calmness_graph_destroy", "pvq_calmness_graph_capacity",
    "pvq_calmness_graph_push", "pvq_calmness_graph_mesh", "pvq_panel_topology", "pvq_panels_batch_create", "pvq_panels_batch_destroy",
    "pvq_panels_batch_graph_capacity", "pvq_panels_batch_rows_device", "pvq_panels_batch_graph_device", "pvq_panels_batch_get_history",
    "pvq_raster_shade", "pvq_raster_touch", "pvq_raster_frame", "pvq_raster_batch_create", "pvq_raster_batch_destroy",
    "pvq_raster_batch_frames_device", "pvq_raster_batch_get_times",
    "pvq_backdrop_geometry", "pvq_backdrop_panel_transforms", "pvq_backdrop_draw_mesh", "pvq_backdrop_frame", "pvq_backdrop_batch_create",
    "pvq_backdrop_batch_destroy", "pvq_backdrop_batch_frames_device", "pvq_backdrop_balls_over_device",
    "pvq_msaa_sample_positions", "pvq_msaa_draw_mesh", "pvq_msaa_frame", "pvq_msaa_batch_create", "pvq_msaa_batch_samples",
    "pvq_overlay_quad", "pvq_overlay_state_create", "pvq_overlay_state_destroy", "pvq_overlay_state_push", "pvq_overlay_state_texture",
    "pvq_overlay_frame", "pvq_overlay_batch_create", "pvq_overlay_batch_destroy", "pvq_overlay_batch_frames_device",
    "pvq_overlay_batch_get_texture",
    "pvq_text_font_from_ttf", "pvq_text_font_from_outlines", "pvq_text_font_destroy", "pvq_text_font_metrics", "pvq_text_font_glyph",
    "pvq_text_pitch_labels", "pvq_text_layout_query", "pvq_text_frame", "pvq_text_batch_create", "pvq_text_batch_destroy",
    "pvq_text_batch_rows_device", "pvq_text_batch_get_coverage",
    "pvq_readout_text", "pvq_readout_layout_query", "pvq_readout_frame", "pvq_readout_batch_create", "pvq_readout_batch_destroy",
    "pvq_readout_batch_rows_device", "pvq_readout_batch_get_atlas",
    "pvq_present_default_settings", "pvq_present_mips", "pvq_present_blend_factors", "pvq_present_frame", "pvq_present_batch_create",
    "pvq_present_batch_destroy", "pvq_present_batch_set_workspace_limit", "pvq_present_batch_rows_device",
    "pvq_synth_bank_create", "pvq_synth_bank_destroy", "pvq_synth_bank_counts", "pvq_synth_state_create", "pvq_synth_state_destroy",
    "pvq_synth_state_render", "pvq_synth_state_get_snapshots", "pvq_synth_state_get_plan", "pvq_synth_state_active_voices",
    "pvq_synth_batch_create", "pvq_synth_batch_destroy", "pvq_synth_batch_render_device", "pvq_synth_batch_get_snapshots", "pvq_synth_batch_last_times",
    "pvq_synth_state_create_ex", "pvq_synth_batch_create_ex", "pvq_synth_state_get_sends", "pvq_synth_effects_create", "pvq_synth_effects_destroy",
    "pvq_synth_effects_process", "pvq_synth_chorus_table",
    "pvq_note_model_create", "pvq_note_model_destroy", "pvq_note_model_sizes", "pvq_note_model_infer", "pvq_note_model_rows_device",
    "pvq_note_model_set_workspace_limit", "pvq_note_model_create_precision", "pvq_note_model_precision", "pvq_note_round",
    "pvq_note_carry_create", "pvq_note_carry_destroy", "pvq_note_carry_reset", "pvq_note_carry_frames_seen", "pvq_note_model_rows_carry_device",
    "pvq_note_trainer_hyper_default", "pvq_note_trainer_create", "pvq_note_trainer_destroy", "pvq_note_trainer_step", "pvq_note_trainer_steps",
    "pvq_note_trainer_param_count", "pvq_note_trainer_read", "pvq_note_trainer_dropout_keep", "pvq_note_trainer_test", "pvq_note_test_metrics",
    "pvq_note_trainer_create_precision", "pvq_note_trainer_precision",
    "pvq_note_trainer_epoch", "pvq_note_epoch_order", "pvq_note_trainer_write", "pvq_note_trainer_set_steps",
    "pvq_vqt_input_status", "pvq_vqt_last_gemm_flop", "pvq_vqt_last_sclk_mhz",
    "pvq_vqt_bandwidths_3db", "pvq_vqt_warning_count", "pvq_vqt_warning",
]

PVQ_OK = 0
PVQ_ERR_ABOVE_NYQUIST = 1
PVQ_ERR_WINDOW_EXCEEDS_NFFT = 2
PVQ_ERR_BAD_LENGTH = 3
PVQ_ERR_INVALID_ARG = 4
PVQ_ERR_NO_DEVICE = 5
PVQ_ERR_DEVICE = 6
PVQ_ERR_UNSUPPORTED = 7
PVQ_ERR_INTERNAL = 8
PVQ_ERR_NONFINITE_INPUT = 9

ALGO_AUTO, ALGO_FFT, ALGO_BLOCKDFT = 0, 1, 2
GEMM_F32, GEMM_BF16X3 = 0, 1
SPECTROGRAM_VQT, SPECTROGRAM_PEAKS = 0, 1
VISUALS_FULL, VISUALS_ZEN, VISUALS_PERFORMANCE, VISUALS_GALAXY = 0, 1, 2, 3   # pvq_visuals_mode
TRAIN_STEP, TRAIN_GRAD, TRAIN_EVAL = 0, 1, 2                      # pvq_train_mode
TRAIN_WEIGHTS, TRAIN_GRADS, TRAIN_ADAM_M, TRAIN_ADAM_V = 0, 1, 2, 3   # pvq_train_array


class CParams(C.Structure):
    _fields_ = [
        ("sr", C.c_float),
        ("n_fft", C.c_uint32),
        ("min_freq", C.c_float),
        ("octaves", C.c_uint32),
        ("buckets_per_octave", C.c_uint32),
        ("sparsity_quantile", C.c_float),
        ("quality", C.c_float),
        ("gamma", C.c_float),
    ]


class CAnalysisParams(C.Structure):
    _fields_ = [
        ("peak_min_prominence", C.c_float),
        ("peak_min_height", C.c_float),
        ("bass_min_prominence", C.c_float),
        ("bass_min_height", C.c_float),
        ("highest_bassnote", C.c_uint32),
        ("harmonic_threshold", C.c_float),
    ]


class CAnalysisBatchOutputs(C.Structure):   # pvq_analysis_batch_outputs (device pointers)
    _fields_ = [(n, C.c_void_p) for n in ("x_vqt_smoothed", "x_vqt_peakfiltered", "x_vqt_afterglow", "calmness", "pitch_accuracy",
                                          "pitch_deviation", "peak_mask", "peak_count", "center", "size")] + \
               [("max_peaks", C.c_uint32), ("scene_calmness", C.c_void_p), ("tuning_grid_inaccuracy", C.c_void_p)]


class CRenderOutputs(C.Structure):   # pvq_render_outputs (device pointers)
    _fields_ = [(n, C.c_void_p) for n in ("spectrogram_vqt", "spectrogram_peaks", "chroma", "led")]


class CSceneSettings(C.Structure):   # pvq_scene_settings
    _fields_ = [("visuals_mode", C.c_int), ("enable_bloom", C.c_int), ("colors", C.POINTER(C.c_float)), ("gray_level", C.c_float),
                ("easing_pow", C.c_float)]


class CSceneInputs(C.Structure):   # pvq_scene_inputs (device pointers)
    _fields_ = [("center", C.c_void_p), ("size", C.c_void_p), ("peak_count", C.c_void_p), ("max_peaks", C.c_uint32),
                ("calmness", C.c_void_p), ("pitch_accuracy", C.c_void_p), ("pitch_deviation", C.c_void_p), ("scene_calmness", C.c_void_p)]


class CSceneOutputs(C.Structure):   # pvq_scene_outputs (device pointers)
    _fields_ = [(n, C.c_void_p) for n in ("ball_xyzs", "ball_rgba", "ball_params", "ball_visible", "bass_lit", "bass_rgba", "bloom")]


class CPanelsOutputs(C.Structure):   # pvq_panels_outputs (device pointers)
    _fields_ = [(n, C.c_void_p) for n in ("line_pos", "line_rgba", "disc_pos", "disc_rgba", "hist_pos", "hist_rgba")]


class CRasterInputs(C.Structure):   # pvq_raster_inputs (device pointers)
    _fields_ = [("ball_xyzs", C.c_void_p), ("ball_rgba", C.c_void_p), ("ball_params", C.c_void_p), ("ball_visible", C.c_void_p),
                ("center", C.c_void_p), ("peak_count", C.c_void_p), ("max_peaks", C.c_uint32), ("background", C.c_void_p)]


class CBackdropPanels(C.Structure):   # pvq_backdrop_panels (host pointers, one row)
    _fields_ = [("line_pos", C.c_void_p), ("line_rgba", C.c_void_p), ("disc_pos", C.c_void_p), ("disc_rgba", C.c_void_p), ("n_peaks", C.c_uint32),
                ("hist_pos", C.c_void_p), ("hist_rgba", C.c_void_p), ("graph_pos", C.c_void_p), ("graph_rgba", C.c_void_p),
                ("graph_capacity", C.c_uint32), ("spectrum_transform", C.c_float * 4), ("histogram_transform", C.c_float * 4),
                ("graph_transform", C.c_float * 4)]


class CBackdropInputs(C.Structure):   # pvq_backdrop_inputs (device pointers)
    _fields_ = [("bass_lit", C.c_void_p), ("bass_rgba", C.c_void_p), ("line_pos", C.c_void_p), ("line_rgba", C.c_void_p),
                ("disc_pos", C.c_void_p), ("disc_rgba", C.c_void_p), ("peak_count", C.c_void_p), ("max_peaks", C.c_uint32),
                ("hist_pos", C.c_void_p), ("hist_rgba", C.c_void_p), ("graph_pos", C.c_void_p), ("graph_rgba", C.c_void_p),
                ("graph_capacity", C.c_uint32), ("spectrum_transform", C.c_float * 4), ("histogram_transform", C.c_float * 4),
                ("graph_transform", C.c_float * 4), ("background", C.c_void_p)]


class CPresentSettings(C.Structure):   # pvq_present_settings
    _fields_ = [(n, C.c_float) for n in ("low_frequency_boost", "low_frequency_boost_curvature", "high_pass_frequency", "threshold",
                                         "threshold_softness")] + \
               [("composite_mode", C.c_int), ("max_mip_dimension", C.c_uint32), ("tonemapping", C.c_int)]


class CTextLabel(C.Structure):   # pvq_text_label
    _fields_ = [("text", C.c_char * 36), ("x", C.c_float), ("y", C.c_float), ("font_px", C.c_float), ("scale", C.c_float), ("rgb", C.c_float * 3)]


class CTextLayout(C.Structure):   # pvq_text_layout
    _fields_ = [("on_image", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32), ("n_segments", C.c_uint32),
                ("n_tiles", C.c_uint32), ("origin_x", C.c_float), ("baseline_y", C.c_float)]


READOUT_MAX_SLOTS = 25   # PVQ_READOUT_MAX_SLOTS


class CReadoutLayout(C.Structure):   # pvq_readout_layout
    _fields_ = [(n, C.c_float) for n in ("xl", "xr", "yt", "yb", "text_width", "font_px", "baseline")] + \
               [("baseline_row", C.c_int32), ("n_slots", C.c_uint32), ("text", C.c_char * (READOUT_MAX_SLOTS + 3))] + \
               [(n, C.c_int32 * READOUT_MAX_SLOTS) for n in ("origin_x", "cell_x0", "cell_y0")] + \
               [(n, C.c_uint32 * READOUT_MAX_SLOTS) for n in ("cell_w", "cell_h")] + \
               [("value_srgb", C.c_float * 3), ("value_linear", C.c_float * 3)]


class CSynthRecord(C.Structure):   # pvq_synth_record
    _fields_ = [("voice", C.c_uint32), ("flags", C.c_uint32), ("ratio_lo", C.c_uint32), ("ratio_hi", C.c_uint32), ("a", C.c_float * 5),
                ("gain", C.c_float * 4), ("desc", C.c_uint32), ("key", C.c_int32), ("stage", C.c_uint32)]


class CSynthSends(C.Structure):   # pvq_synth_sends
    _fields_ = [("chorus", C.c_float * 4), ("reverb", C.c_float * 2), ("pad", C.c_uint32 * 2)]


class CNoteModelParams(C.Structure):   # pvq_note_model_params
    _fields_ = [(n, C.c_uint32) for n in ("n_bins", "t_frames", "mlp_size", "mlp_layers")]


class CNoteModelWeights(C.Structure):   # pvq_note_model_weights (host pointers)
    _fields_ = [("conv_weight", C.POINTER(C.c_float)), ("conv_bias", C.POINTER(C.c_float)), ("fc1_weight", C.POINTER(C.c_float)),
                ("fc1_bias", C.POINTER(C.c_float)), ("layer_weight", C.POINTER(C.POINTER(C.c_float))),
                ("layer_bias", C.POINTER(C.POINTER(C.c_float))), ("output_weight", C.POINTER(C.c_float)),
                ("output_bias", C.POINTER(C.c_float))]


class CNoteModelOutputs(C.Structure):   # pvq_note_model_outputs (device pointers)
    _fields_ = [(n, C.c_void_p) for n in ("d_prob", "d_logits", "d_mask")]


class CNoteTrainerHyper(C.Structure):   # pvq_note_trainer_hyper
    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "dropout")] + [("seed", C.c_uint64)]


class CNoteTestBatch(C.Structure):   # pvq_note_test_batch
    _fields_ = [(n, C.c_uint32) for n in ("rows", "tp", "fp", "fn", "correct", "_pad")] + [("loss", C.c_double)]


class CShard(C.Structure):   # pvq_shard
    _fields_ = [("first_frame", C.c_uint64), ("n_frames", C.c_uint64), ("sample_begin", C.c_uint64), ("sample_end", C.c_uint64),
                ("n_lead", C.c_uint64)]


class CAnalysisFullParams(C.Structure):
    _fields_ = [
        ("spectrogram_length", C.c_uint32),
        ("peak_min_prominence", C.c_float), ("peak_min_height", C.c_float),
        ("bass_min_prominence", C.c_float), ("bass_min_height", C.c_float),
        ("highest_bassnote", C.c_uint32),
        ("vqt_smoothing_duration_base_ns", C.c_uint64),
        ("vqt_smoothing_calmness_min", C.c_float), ("vqt_smoothing_calmness_max", C.c_float),
        ("note_calmness_smoothing_duration_ns", C.c_uint64),
        ("scene_calmness_smoothing_duration_ns", C.c_uint64),
        ("tuning_inaccuracy_smoothing_duration_ns", C.c_uint64),
        ("harmonic_threshold", C.c_float),
    ]


_lib = None


def load():
    """Load libpvq.so; raise (never fall back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C pitchvis_amd/csrc` (or "
            "`python -c 'import __graft_entry__ as g; g.build()'`).  pitchvis_amd has no CPU fallback."
        )
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.  Both HIP
    # runtimes in one process do not coexist (whichever initialises second sees no GPU), and the
    # dynamic loader de-duplicates by SONAME, so: let torch's copy load first whenever torch is
    # installed; libpvq then binds to that same runtime.  Without torch the system ROCm runtime
    # is used.  (torch is plumbing here: device memory, streams, torch.distributed.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    fp, up, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
    L.pvq_status_string.argtypes = [C.c_int]; L.pvq_status_string.restype = C.c_char_p
    L.pvq_last_error.argtypes = []; L.pvq_last_error.restype = C.c_char_p
    L.pvq_abi_version.argtypes = []; L.pvq_abi_version.restype = C.c_uint32
    L.pvq_vqt_default_params.argtypes = [C.POINTER(CParams)]
    L.pvq_vqt_create.argtypes = [C.POINTER(CParams), C.c_int, C.POINTER(vp), fp]; L.pvq_vqt_create.restype = C.c_int
    L.pvq_vqt_destroy.argtypes = [vp]
    L.pvq_vqt_get_params.argtypes = [vp, C.POINTER(CParams)]
    L.pvq_vqt_n_bins.argtypes = [vp]; L.pvq_vqt_n_bins.restype = C.c_uint32
    L.pvq_vqt_delay_seconds.argtypes = [vp]; L.pvq_vqt_delay_seconds.restype = C.c_double
    L.pvq_vqt_window_union.argtypes = [vp]; L.pvq_vqt_window_union.restype = C.c_uint32
    L.pvq_vqt_bandwidths_3db.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]; L.pvq_vqt_bandwidths_3db.restype = C.c_int
    L.pvq_vqt_warning_count.argtypes = [vp]; L.pvq_vqt_warning_count.restype = C.c_uint32
    L.pvq_vqt_warning.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]; L.pvq_vqt_warning.restype = C.c_int
    L.pvq_vqt_n_groups.argtypes = [vp]; L.pvq_vqt_n_groups.restype = C.c_uint32
    L.pvq_vqt_group_info.argtypes = [vp, C.c_uint32, up]; L.pvq_vqt_group_info.restype = C.c_int
    L.pvq_vqt_group_csr.argtypes = [vp, C.c_uint32, C.c_int, up, up, fp]; L.pvq_vqt_group_csr.restype = C.c_int
    L.pvq_vqt_filter_params.argtypes = [vp, fp, fp, up, up]; L.pvq_vqt_filter_params.restype = C.c_int
    L.pvq_vqt_calculate_instant_db.argtypes = [vp, fp, C.c_size_t, fp]; L.pvq_vqt_calculate_instant_db.restype = C.c_int
    L.pvq_vqt_calculate_batch_db.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_size_t, fp]
    L.pvq_vqt_calculate_batch_db.restype = C.c_int
    L.pvq_vqt_calculate_batch_db_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, vp]
    L.pvq_vqt_calculate_batch_db_device.restype = C.c_int
    L.pvq_vqt_set_algo.argtypes = [vp, C.c_int]; L.pvq_vqt_set_algo.restype = C.c_int
    L.pvq_vqt_last_algo.argtypes = [vp]; L.pvq_vqt_last_algo.restype = C.c_int
    L.pvq_vqt_resolve_algo.argtypes = [vp, C.c_size_t, C.c_size_t]; L.pvq_vqt_resolve_algo.restype = C.c_int
    L.pvq_vqt_blockdft_columns.argtypes = [vp]; L.pvq_vqt_blockdft_columns.restype = C.c_uint32
    L.pvq_vqt_set_gemm_precision.argtypes = [vp, C.c_int]; L.pvq_vqt_set_gemm_precision.restype = C.c_int
    L.pvq_vqt_set_workspace_limit.argtypes = [vp, C.c_uint64]; L.pvq_vqt_set_workspace_limit.restype = C.c_int
    L.pvq_analysis_default_params.argtypes = [C.POINTER(CAnalysisParams)]
    L.pvq_analyze_batch_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(CAnalysisParams), vp, vp, vp, vp, C.c_uint32, vp]
    L.pvq_analyze_batch_device.restype = C.c_int
    L.pvq_analyze_batch.argtypes = [vp, fp, C.c_size_t, C.POINTER(CAnalysisParams), up, up, fp, fp, C.c_uint32]
    L.pvq_analyze_batch.restype = C.c_int
    L.pvq_vqt_analyze_batch_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(CAnalysisParams),
                                               vp, vp, vp, vp, vp, C.c_uint32, vp]
    L.pvq_vqt_analyze_batch_device.restype = C.c_int
    szp = C.POINTER(C.c_size_t)
    L.pvq_vqt_calculate_batch_db_streams.argtypes = [vp, C.POINTER(vp), szp, szp, C.c_uint32, C.c_size_t, vp, C.c_size_t, vp]
    L.pvq_vqt_calculate_batch_db_streams.restype = C.c_int
    L.pvq_vqt_analyze_batch_streams.argtypes = [vp, C.POINTER(vp), szp, szp, C.c_uint32, C.c_size_t, C.POINTER(CAnalysisParams), vp, C.c_size_t,
                                                vp, vp, vp, vp, C.c_uint32, vp]
    L.pvq_vqt_analyze_batch_streams.restype = C.c_int
    L.pvq_plan_shard.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(CShard)]; L.pvq_plan_shard.restype = C.c_int
    L.pvq_vqt_analyze_batch_multi.argtypes = [C.POINTER(vp), C.c_uint32, fp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(CAnalysisParams),
                                              fp, up, up, fp, fp, C.c_uint32]
    L.pvq_vqt_analyze_batch_multi.restype = C.c_int
    L.pvq_vqt_set_profiling.argtypes = [vp, C.c_int]; L.pvq_vqt_set_profiling.restype = C.c_int
    L.pvq_vqt_last_kernel_ms.argtypes = [vp, fp, C.c_uint32]; L.pvq_vqt_last_kernel_ms.restype = C.c_uint32
    L.pvq_vqt_last_kernel_launches.argtypes = [vp, up, C.c_uint32]; L.pvq_vqt_last_kernel_launches.restype = C.c_uint32
    L.pvq_vqt_last_frames_per_launch.argtypes = [vp]; L.pvq_vqt_last_frames_per_launch.restype = C.c_uint32
    L.pvq_vqt_kernel_name.argtypes = [C.c_uint32]; L.pvq_vqt_kernel_name.restype = C.c_char_p
    afp = C.POINTER(CAnalysisFullParams)
    L.pvq_analysis_full_default_params.argtypes = [afp]
    L.pvq_analysis_state_create.argtypes = [C.c_float, C.c_uint32, C.c_uint32, afp, C.POINTER(vp)]
    L.pvq_analysis_state_create.restype = C.c_int
    L.pvq_analysis_batch_create.argtypes = [C.c_int, C.c_float, C.c_uint32, C.c_uint32, afp, C.c_uint32, C.POINTER(vp)]; L.pvq_analysis_batch_create.restype = C.c_int
    L.pvq_analysis_batch_destroy.argtypes = [vp]
    L.pvq_analysis_batch_update_vqt_smoothing_duration.argtypes = [vp, C.c_int, C.c_uint64]; L.pvq_analysis_batch_update_vqt_smoothing_duration.restype = C.c_int
    L.pvq_analysis_batch_preprocess_device.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(CAnalysisBatchOutputs), vp]
    L.pvq_analysis_batch_preprocess_device.restype = C.c_int
    L.pvq_analysis_batch_preprocess_pcm.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_uint64, vp,
                                                    C.POINTER(CAnalysisBatchOutputs), vp]
    L.pvq_analysis_batch_preprocess_pcm.restype = C.c_int
    L.pvq_analysis_batch_get_field.argtypes = [vp, C.c_uint32, C.c_int, fp]; L.pvq_analysis_batch_get_field.restype = C.c_int
    L.pvq_analysis_batch_get_scalars.argtypes = [vp, C.c_uint32, fp, fp]; L.pvq_analysis_batch_get_scalars.restype = C.c_int
    L.pvq_analysis_state_destroy.argtypes = [vp]
    L.pvq_analysis_state_update_vqt_smoothing_duration.argtypes = [vp, C.c_int, C.c_uint64]
    L.pvq_analysis_state_update_vqt_smoothing_duration.restype = C.c_int
    L.pvq_analysis_state_preprocess.argtypes = [vp, fp, C.c_size_t, C.c_uint64]; L.pvq_analysis_state_preprocess.restype = C.c_int
    L.pvq_analysis_state_bin_to_frequency.argtypes = [vp, C.c_uint32]; L.pvq_analysis_state_bin_to_frequency.restype = C.c_float
    L.pvq_analysis_state_n_buckets.argtypes = [vp]; L.pvq_analysis_state_n_buckets.restype = C.c_uint32
    L.pvq_analysis_state_get_field.argtypes = [vp, C.c_int, fp]; L.pvq_analysis_state_get_field.restype = C.c_int
    L.pvq_analysis_state_get_peaks.argtypes = [vp, up, C.c_uint32]; L.pvq_analysis_state_get_peaks.restype = C.c_uint32
    L.pvq_analysis_state_get_peaks_continuous.argtypes = [vp, fp, fp, C.c_uint32]
    L.pvq_analysis_state_get_peaks_continuous.restype = C.c_uint32
    L.pvq_analysis_state_scene_calmness.argtypes = [vp]; L.pvq_analysis_state_scene_calmness.restype = C.c_float
    L.pvq_analysis_state_tuning_grid_inaccuracy.argtypes = [vp]; L.pvq_analysis_state_tuning_grid_inaccuracy.restype = C.c_float
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.pvq_vqt_set_twiddle_fp16.argtypes = [vp, C.c_int]; L.pvq_vqt_set_twiddle_fp16.restype = C.c_int
    L.pvq_mono_agc_create.argtypes = [C.c_float, C.c_float, C.POINTER(vp)]; L.pvq_mono_agc_create.restype = C.c_int
    L.pvq_mono_agc_destroy.argtypes = [vp]
    L.pvq_mono_agc_freeze_gain.argtypes = [vp, C.c_int]
    L.pvq_mono_agc_is_gain_frozen.argtypes = [vp]; L.pvq_mono_agc_is_gain_frozen.restype = C.c_int
    L.pvq_mono_agc_gain.argtypes = [vp]; L.pvq_mono_agc_gain.restype = C.c_float
    L.pvq_mono_agc_process.argtypes = [vp, fp, C.c_size_t]
    L.pvq_train_chunk_samples.argtypes = [vp]; L.pvq_train_chunk_samples.restype = C.c_size_t
    L.pvq_train_condition_stream.argtypes = [vp, fp, fp, C.c_size_t, C.c_size_t, fp, fp]
    L.pvq_train_condition_stream.restype = C.c_int
    L.pvq_agc_batch_create.argtypes = [C.c_int, C.c_uint32, C.c_float, C.c_float, C.POINTER(vp)]; L.pvq_agc_batch_create.restype = C.c_int
    L.pvq_agc_batch_destroy.argtypes = [vp]
    L.pvq_agc_batch_condition_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), szp, C.c_size_t, C.POINTER(vp), vp, C.c_size_t, vp]
    L.pvq_agc_batch_condition_device.restype = C.c_int
    L.pvq_agc_batch_get_gains.argtypes = [vp, fp]; L.pvq_agc_batch_get_gains.restype = C.c_int
    L.pvq_train_frames_db.argtypes = [vp, fp, C.c_size_t, C.c_size_t, C.c_size_t, fp]; L.pvq_train_frames_db.restype = C.c_int
    L.pvq_train_rows.argtypes = [fp, C.c_size_t, C.c_uint32, up, ip, fp, fp, fp, fp]; L.pvq_train_rows.restype = C.c_int
    L.pvq_npy_write_f32.argtypes = [C.c_char_p, fp, C.c_uint64]; L.pvq_npy_write_f32.restype = C.c_int
    L.pvq_stream_create.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(vp)]; L.pvq_stream_create.restype = C.c_int
    L.pvq_stream_destroy.argtypes = [vp]
    L.pvq_stream_push.argtypes = [vp, fp, C.c_size_t]; L.pvq_stream_push.restype = C.c_int
    L.pvq_stream_gain.argtypes = [vp]; L.pvq_stream_gain.restype = C.c_float
    L.pvq_stream_chunk_size_ms.argtypes = [vp]; L.pvq_stream_chunk_size_ms.restype = C.c_float
    L.pvq_stream_frame_db.argtypes = [vp, fp]; L.pvq_stream_frame_db.restype = C.c_int
    L.pvq_stream_read.argtypes = [vp, fp, C.c_size_t]; L.pvq_stream_read.restype = C.c_int
    L.pvq_calculate_color.argtypes = [C.c_uint16, C.c_float, fp, C.c_float, C.c_float, fp]
    L.pvq_led_frame.argtypes = [C.c_uint32, C.c_uint16, fp, fp, C.c_uint32, fp, C.c_float, C.c_float, bp]
    L.pvq_led_frame.restype = C.c_size_t
    L.pvq_spectrogram_row.argtypes = [C.c_int, C.c_uint32, C.c_uint16, fp, fp, fp, C.c_uint32, fp, C.c_float, C.c_float, bp]
    L.pvq_spectrogram_row.restype = C.c_int
    L.pvq_chroma_row.argtypes = [C.c_float, C.c_uint32, C.c_uint16, fp, fp]; L.pvq_chroma_row.restype = C.c_int
    L.pvq_render_batch_create.argtypes = [C.c_int, C.c_float, C.c_uint32, C.c_uint32, fp, C.c_float, C.c_float, C.POINTER(vp)]
    L.pvq_render_batch_create.restype = C.c_int
    L.pvq_render_batch_destroy.argtypes = [vp]
    L.pvq_render_batch_rows_device.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, C.c_uint32, C.POINTER(CRenderOutputs), vp]
    L.pvq_render_batch_rows_device.restype = C.c_int
    ssp = C.POINTER(CSceneSettings)
    L.pvq_scene_default_settings.argtypes = [ssp]; L.pvq_scene_default_settings.restype = None
    L.pvq_scene_state_create.argtypes = [C.c_uint32, C.c_uint32, ssp, C.POINTER(vp)]; L.pvq_scene_state_create.restype = C.c_int
    L.pvq_scene_state_destroy.argtypes = [vp]; L.pvq_scene_state_destroy.restype = None
    L.pvq_scene_state_n_bins.argtypes = [vp]; L.pvq_scene_state_n_bins.restype = C.c_uint32
    L.pvq_scene_state_n_segments.argtypes = [vp]; L.pvq_scene_state_n_segments.restype = C.c_uint32
    L.pvq_scene_state_update.argtypes = [vp, fp, fp, C.c_uint32, fp, fp, fp, C.c_float, C.c_uint64]; L.pvq_scene_state_update.restype = C.c_int
    L.pvq_scene_state_get.argtypes = [vp, fp, fp, fp, up, up, fp, fp]; L.pvq_scene_state_get.restype = C.c_int
    L.pvq_scene_batch_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, ssp, C.c_uint32, C.POINTER(vp)]; L.pvq_scene_batch_create.restype = C.c_int
    L.pvq_scene_batch_destroy.argtypes = [vp]; L.pvq_scene_batch_destroy.restype = None
    L.pvq_scene_batch_n_segments.argtypes = [vp]; L.pvq_scene_batch_n_segments.restype = C.c_uint32
    L.pvq_scene_batch_frames_device.argtypes = [vp, C.c_size_t, C.POINTER(CSceneInputs), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(CSceneOutputs), vp]
    L.pvq_scene_batch_frames_device.restype = C.c_int
    L.pvq_scene_batch_get_state.argtypes = [vp, C.c_uint32, fp, fp, fp, up, up, fp, fp]; L.pvq_scene_batch_get_state.restype = C.c_int
    if not _dev or _dev == "1" or hasattr(L, "pvq_ml_midi_pitch"):   # (as for pvq_msaa_frame below)
        L.pvq_ml_scene_state_update.argtypes = [vp, fp, fp, C.c_uint32, fp, fp, fp, C.c_float, C.c_uint64, fp]; L.pvq_ml_scene_state_update.restype = C.c_int
        L.pvq_ml_midi_pitch.argtypes = [C.c_uint32, C.c_uint32, up]; L.pvq_ml_midi_pitch.restype = C.c_int
        L.pvq_ml_scene_batch_frames_device.argtypes = [vp, C.c_size_t, C.POINTER(CSceneInputs), vp, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64),
                                                       C.POINTER(CSceneOutputs), vp]
        L.pvq_ml_scene_batch_frames_device.restype = C.c_int
    L.pvq_spectrum_mesh.argtypes = [C.c_uint32, C.c_uint16, fp, fp, fp, C.c_uint32, fp, C.c_float, fp, fp, fp, fp]; L.pvq_spectrum_mesh.restype = C.c_int
    L.pvq_calmness_histogram_mesh.argtypes = [C.c_uint32, fp, fp, fp]; L.pvq_calmness_histogram_mesh.restype = C.c_int
    L.pvq_calmness_graph_create.argtypes = [C.c_uint32, C.POINTER(vp)]; L.pvq_calmness_graph_create.restype = C.c_int
    L.pvq_calmness_graph_destroy.argtypes = [vp]; L.pvq_calmness_graph_destroy.restype = None
    L.pvq_calmness_graph_capacity.argtypes = [vp]; L.pvq_calmness_graph_capacity.restype = C.c_uint32
    L.pvq_calmness_graph_push.argtypes = [vp, C.c_float]; L.pvq_calmness_graph_push.restype = C.c_int
    L.pvq_calmness_graph_mesh.argtypes = [vp, fp, fp, fp]; L.pvq_calmness_graph_mesh.restype = C.c_int
    L.pvq_panel_topology.argtypes = [C.c_uint32, C.c_uint32, up, fp]; L.pvq_panel_topology.restype = C.c_int
    L.pvq_panels_batch_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, fp, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pvq_panels_batch_create.restype = C.c_int
    L.pvq_panels_batch_destroy.argtypes = [vp]; L.pvq_panels_batch_destroy.restype = None
    L.pvq_panels_batch_graph_capacity.argtypes = [vp]; L.pvq_panels_batch_graph_capacity.restype = C.c_uint32
    L.pvq_panels_batch_rows_device.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, C.c_uint32, vp, C.POINTER(CPanelsOutputs), vp]
    L.pvq_panels_batch_rows_device.restype = C.c_int
    L.pvq_panels_batch_graph_device.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp]; L.pvq_panels_batch_graph_device.restype = C.c_int
    L.pvq_panels_batch_get_history.argtypes = [vp, C.c_uint32, fp]; L.pvq_panels_batch_get_history.restype = C.c_int
    L.pvq_raster_shade.argtypes = [fp, fp, C.c_float, C.c_float, fp]; L.pvq_raster_shade.restype = C.c_int
    L.pvq_raster_touch.argtypes = [C.c_uint32, fp, C.c_uint32, C.c_float, fp]; L.pvq_raster_touch.restype = C.c_int
    L.pvq_raster_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, fp, fp, fp, up, fp, fp, fp]; L.pvq_raster_frame.restype = C.c_int
    L.pvq_raster_batch_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pvq_raster_batch_create.restype = C.c_int
    L.pvq_raster_batch_destroy.argtypes = [vp]; L.pvq_raster_batch_destroy.restype = None
    L.pvq_raster_batch_frames_device.argtypes = [vp, C.c_size_t, C.POINTER(CRasterInputs), fp, vp, vp, vp]; L.pvq_raster_batch_frames_device.restype = C.c_int
    L.pvq_raster_batch_get_times.argtypes = [vp, C.c_uint32, fp]; L.pvq_raster_batch_get_times.restype = C.c_int
    L.pvq_backdrop_geometry.argtypes = [C.c_uint32, C.c_int, fp, up]; L.pvq_backdrop_geometry.restype = C.c_int
    L.pvq_backdrop_panel_transforms.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, fp]; L.pvq_backdrop_panel_transforms.restype = C.c_int
    L.pvq_backdrop_draw_mesh.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_size_t, fp, fp, fp, fp]; L.pvq_backdrop_draw_mesh.restype = C.c_int
    L.pvq_backdrop_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_uint32, fp, C.POINTER(CBackdropPanels),
                                     fp, fp]
    L.pvq_backdrop_frame.restype = C.c_int
    L.pvq_backdrop_batch_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pvq_backdrop_batch_create.restype = C.c_int
    L.pvq_backdrop_batch_destroy.argtypes = [vp]; L.pvq_backdrop_batch_destroy.restype = None
    L.pvq_backdrop_batch_frames_device.argtypes = [vp, C.c_size_t, C.POINTER(CBackdropInputs), vp, vp]; L.pvq_backdrop_batch_frames_device.restype = C.c_int
    L.pvq_backdrop_balls_over_device.argtypes = [vp, C.c_size_t, C.POINTER(CRasterInputs), fp, vp, vp, vp]; L.pvq_backdrop_balls_over_device.restype = C.c_int
    if not _dev or _dev == "1" or hasattr(L, "pvq_msaa_frame"):   # (a library of older sources kept for an A/B, PVQ_DEV_LIB=<name>, may predate them)
        L.pvq_msaa_sample_positions.argtypes = [C.c_uint32, fp]; L.pvq_msaa_sample_positions.restype = C.c_int
        L.pvq_msaa_draw_mesh.argtypes = [C.c_uint32] + L.pvq_backdrop_draw_mesh.argtypes; L.pvq_msaa_draw_mesh.restype = C.c_int
        L.pvq_msaa_frame.argtypes = [C.c_uint32] + L.pvq_backdrop_frame.argtypes; L.pvq_msaa_frame.restype = C.c_int
        L.pvq_msaa_batch_create.argtypes = [C.c_uint32] + L.pvq_backdrop_batch_create.argtypes; L.pvq_msaa_batch_create.restype = C.c_int
        L.pvq_msaa_batch_samples.argtypes = [vp]; L.pvq_msaa_batch_samples.restype = C.c_uint32
    L.pvq_overlay_quad.argtypes = [C.c_uint32, C.c_uint32, fp]; L.pvq_overlay_quad.restype = C.c_int
    L.pvq_overlay_state_create.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(vp)]; L.pvq_overlay_state_create.restype = C.c_int
    L.pvq_overlay_state_destroy.argtypes = [vp]; L.pvq_overlay_state_destroy.restype = None
    L.pvq_overlay_state_push.argtypes = [vp, bp]; L.pvq_overlay_state_push.restype = C.c_int
    L.pvq_overlay_state_texture.argtypes = [vp, bp, up]; L.pvq_overlay_state_texture.restype = C.c_int
    L.pvq_overlay_frame.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, fp, fp, fp, fp]; L.pvq_overlay_frame.restype = C.c_int
    L.pvq_overlay_batch_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, fp, fp, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.POINTER(vp)]
    L.pvq_overlay_batch_create.restype = C.c_int
    L.pvq_overlay_batch_destroy.argtypes = [vp]; L.pvq_overlay_batch_destroy.restype = None
    L.pvq_overlay_batch_frames_device.argtypes = [vp, C.c_size_t, vp, vp, vp, vp]; L.pvq_overlay_batch_frames_device.restype = C.c_int
    L.pvq_overlay_batch_get_texture.argtypes = [vp, C.c_uint32, bp, up]; L.pvq_overlay_batch_get_texture.restype = C.c_int
    tlp = C.POINTER(CTextLabel)
    L.pvq_text_font_from_ttf.argtypes = [bp, C.c_size_t, C.POINTER(vp)]; L.pvq_text_font_from_ttf.restype = C.c_int
    L.pvq_text_font_from_outlines.argtypes = [C.c_uint32, up, fp, up, up, up, fp, bp, C.c_uint32, C.c_float, C.c_float, C.POINTER(vp)]
    L.pvq_text_font_from_outlines.restype = C.c_int
    L.pvq_text_font_destroy.argtypes = [vp]; L.pvq_text_font_destroy.restype = None
    L.pvq_text_font_metrics.argtypes = [vp, up, fp, fp]; L.pvq_text_font_metrics.restype = C.c_int
    L.pvq_text_font_glyph.argtypes = [vp, C.c_uint32, fp, up, up, C.c_uint32, C.c_uint32, up, fp, bp]; L.pvq_text_font_glyph.restype = C.c_int
    L.pvq_text_pitch_labels.argtypes = [C.c_uint32, fp, tlp]; L.pvq_text_pitch_labels.restype = C.c_int
    L.pvq_text_layout_query.argtypes = [vp, tlp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(CTextLayout)]
    L.pvq_text_layout_query.restype = C.c_int
    L.pvq_text_frame.argtypes = [vp, tlp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, fp, fp]; L.pvq_text_frame.restype = C.c_int
    L.pvq_text_batch_create.argtypes = [C.c_int, vp, tlp, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pvq_text_batch_create.restype = C.c_int
    L.pvq_text_batch_destroy.argtypes = [vp]; L.pvq_text_batch_destroy.restype = None
    L.pvq_text_batch_rows_device.argtypes = [vp, C.c_size_t, vp, vp]; L.pvq_text_batch_rows_device.restype = C.c_int
    L.pvq_text_batch_get_coverage.argtypes = [vp, C.c_int, fp]; L.pvq_text_batch_get_coverage.restype = C.c_int
    ip = C.POINTER(C.c_int32)
    L.pvq_readout_text.argtypes = [C.c_float, C.c_char_p, fp]; L.pvq_readout_text.restype = C.c_int
    L.pvq_readout_layout_query.argtypes = [vp, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(CReadoutLayout)]
    L.pvq_readout_layout_query.restype = C.c_int
    L.pvq_readout_frame.argtypes = [vp, C.c_float, C.c_uint32, C.c_uint32, C.c_float, fp]; L.pvq_readout_frame.restype = C.c_int
    L.pvq_readout_batch_create.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(vp)]; L.pvq_readout_batch_create.restype = C.c_int
    L.pvq_readout_batch_destroy.argtypes = [vp]; L.pvq_readout_batch_destroy.restype = None
    L.pvq_readout_batch_rows_device.argtypes = [vp, C.c_size_t, vp, vp, vp]; L.pvq_readout_batch_rows_device.restype = C.c_int
    L.pvq_readout_batch_get_atlas.argtypes = [vp, C.c_uint32, ip, ip, up, up, fp, C.c_size_t, fp]; L.pvq_readout_batch_get_atlas.restype = C.c_int
    psp = C.POINTER(CPresentSettings)
    L.pvq_present_default_settings.argtypes = [psp]; L.pvq_present_default_settings.restype = None
    L.pvq_present_mips.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, up, up]; L.pvq_present_mips.restype = C.c_int
    L.pvq_present_blend_factors.argtypes = [psp, C.c_float, C.c_uint32, fp]; L.pvq_present_blend_factors.restype = C.c_int
    L.pvq_present_frame.argtypes = [psp, C.c_uint32, C.c_uint32, fp, C.c_float, bp, fp]; L.pvq_present_frame.restype = C.c_int
    L.pvq_present_batch_create.argtypes = [C.c_int, psp, C.c_uint32, C.c_uint32, C.POINTER(vp)]; L.pvq_present_batch_create.restype = C.c_int
    L.pvq_present_batch_destroy.argtypes = [vp]; L.pvq_present_batch_destroy.restype = None
    L.pvq_present_batch_set_workspace_limit.argtypes = [vp, C.c_uint64]; L.pvq_present_batch_set_workspace_limit.restype = C.c_int
    L.pvq_present_batch_rows_device.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, vp]; L.pvq_present_batch_rows_device.restype = C.c_int
    i16p, i32p, u64p, dp_ = C.POINTER(C.c_int16), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    L.pvq_synth_bank_create.argtypes = [i16p, C.c_size_t, i32p, C.c_uint32, i16p, up, C.c_uint32, up, C.c_uint32, i16p, up, C.c_uint32, i32p, C.c_uint32,
                                        C.POINTER(vp)]
    L.pvq_synth_bank_create.restype = C.c_int
    L.pvq_synth_bank_destroy.argtypes = [vp]; L.pvq_synth_bank_destroy.restype = None
    L.pvq_synth_bank_counts.argtypes = [vp, u64p]; L.pvq_synth_bank_counts.restype = C.c_int
    L.pvq_synth_state_create.argtypes = [vp, C.c_int32, C.c_uint32, C.POINTER(vp)]; L.pvq_synth_state_create.restype = C.c_int
    L.pvq_synth_state_destroy.argtypes = [vp]; L.pvq_synth_state_destroy.restype = None
    L.pvq_synth_state_render.argtypes = [vp, dp_, i32p, i32p, i32p, i32p, C.c_size_t, C.c_size_t, up, C.c_size_t, fp, fp]
    L.pvq_synth_state_render.restype = C.c_int
    L.pvq_synth_state_get_snapshots.argtypes = [vp, up, up, C.c_size_t, i32p, fp, fp, C.c_size_t]; L.pvq_synth_state_get_snapshots.restype = C.c_int
    L.pvq_synth_state_get_plan.argtypes = [vp, up, up, C.c_size_t, C.POINTER(CSynthRecord), C.c_size_t]; L.pvq_synth_state_get_plan.restype = C.c_int
    L.pvq_synth_state_active_voices.argtypes = [vp]; L.pvq_synth_state_active_voices.restype = C.c_uint32
    L.pvq_synth_batch_create.argtypes = [C.c_int, vp, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(vp)]; L.pvq_synth_batch_create.restype = C.c_int
    L.pvq_synth_batch_destroy.argtypes = [vp]; L.pvq_synth_batch_destroy.restype = None
    L.pvq_synth_batch_render_device.argtypes = [vp, u64p, dp_, i32p, i32p, i32p, i32p, szp, C.POINTER(vp), C.POINTER(vp), up, C.c_size_t, vp]
    L.pvq_synth_batch_render_device.restype = C.c_int
    L.pvq_synth_batch_get_snapshots.argtypes = [vp, C.c_uint32, up, up, C.c_size_t, i32p, fp, fp, C.c_size_t]
    L.pvq_synth_batch_get_snapshots.restype = C.c_int
    L.pvq_synth_batch_last_times.argtypes = [vp, fp, u64p]; L.pvq_synth_batch_last_times.restype = C.c_int
    L.pvq_synth_state_create_ex.argtypes = [vp, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(vp)]; L.pvq_synth_state_create_ex.restype = C.c_int
    L.pvq_synth_batch_create_ex.argtypes = [C.c_int, vp, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pvq_synth_batch_create_ex.restype = C.c_int
    L.pvq_synth_state_get_sends.argtypes = [vp, up, up, C.c_size_t, C.POINTER(CSynthSends), C.c_size_t]; L.pvq_synth_state_get_sends.restype = C.c_int
    L.pvq_synth_effects_create.argtypes = [C.c_int32, C.POINTER(vp)]; L.pvq_synth_effects_create.restype = C.c_int
    L.pvq_synth_effects_destroy.argtypes = [vp]; L.pvq_synth_effects_destroy.restype = None
    L.pvq_synth_effects_process.argtypes = [vp, C.c_size_t, fp, fp, fp, fp, fp, fp, fp]; L.pvq_synth_effects_process.restype = C.c_int
    L.pvq_synth_chorus_table.argtypes = [C.c_int32, fp, C.c_size_t]; L.pvq_synth_chorus_table.restype = C.c_uint32
    L.pvq_note_model_create.argtypes = [C.c_int, C.POINTER(CNoteModelParams), C.POINTER(CNoteModelWeights), C.POINTER(vp)]
    L.pvq_note_model_create.restype = C.c_int
    L.pvq_note_model_destroy.argtypes = [vp]
    L.pvq_note_model_sizes.argtypes = [vp, up]; L.pvq_note_model_sizes.restype = C.c_int
    L.pvq_note_model_infer.argtypes = [vp, fp, fp]; L.pvq_note_model_infer.restype = C.c_int
    L.pvq_note_model_rows_device.argtypes = [vp, vp, szp, C.c_uint32, C.c_size_t, C.POINTER(CNoteModelOutputs), vp]
    L.pvq_note_model_rows_device.restype = C.c_int
    L.pvq_note_model_set_workspace_limit.argtypes = [vp, C.c_uint64]; L.pvq_note_model_set_workspace_limit.restype = C.c_int
    if not _dev or _dev == "1" or hasattr(L, "pvq_note_carry_create"):   # (a library of older sources kept for an A/B may predate them)
        L.pvq_note_carry_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]; L.pvq_note_carry_create.restype = C.c_int
        L.pvq_note_carry_destroy.argtypes = [vp]; L.pvq_note_carry_destroy.restype = None
        L.pvq_note_carry_reset.argtypes = [vp, C.c_int64, vp]; L.pvq_note_carry_reset.restype = C.c_int
        L.pvq_note_carry_frames_seen.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64)]; L.pvq_note_carry_frames_seen.restype = C.c_int
        L.pvq_note_model_rows_carry_device.argtypes = [vp, vp, vp, szp, C.c_uint32, C.c_size_t, C.POINTER(CNoteModelOutputs), vp]
        L.pvq_note_model_rows_carry_device.restype = C.c_int
    L.pvq_note_model_create_precision.argtypes = [C.c_int, C.POINTER(CNoteModelParams), C.POINTER(CNoteModelWeights), C.c_int, C.POINTER(vp)]
    L.pvq_note_model_create_precision.restype = C.c_int
    L.pvq_note_model_precision.argtypes = [vp, C.POINTER(C.c_int)]; L.pvq_note_model_precision.restype = C.c_int
    L.pvq_note_round.argtypes = [C.c_int, fp, C.c_size_t, fp]; L.pvq_note_round.restype = C.c_int
    L.pvq_note_trainer_hyper_default.argtypes = [C.POINTER(CNoteTrainerHyper)]; L.pvq_note_trainer_hyper_default.restype = None
    L.pvq_note_trainer_create.argtypes = [C.c_int, C.POINTER(CNoteModelParams), C.POINTER(CNoteModelWeights), C.POINTER(CNoteTrainerHyper), C.c_uint32,
                                          C.POINTER(vp)]
    L.pvq_note_trainer_create.restype = C.c_int
    L.pvq_note_trainer_create_precision.argtypes = [C.c_int, C.POINTER(CNoteModelParams), C.POINTER(CNoteModelWeights), C.POINTER(CNoteTrainerHyper),
                                                    C.c_uint32, C.c_int, C.POINTER(vp)]
    L.pvq_note_trainer_create_precision.restype = C.c_int
    L.pvq_note_trainer_precision.argtypes = [vp]; L.pvq_note_trainer_precision.restype = C.c_int
    L.pvq_note_trainer_destroy.argtypes = [vp]; L.pvq_note_trainer_destroy.restype = None
    L.pvq_note_trainer_step.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, up, C.c_uint32, vp, vp, vp]; L.pvq_note_trainer_step.restype = C.c_int
    L.pvq_note_trainer_steps.argtypes = [vp]; L.pvq_note_trainer_steps.restype = C.c_uint64
    L.pvq_note_trainer_param_count.argtypes = [vp]; L.pvq_note_trainer_param_count.restype = C.c_uint64
    L.pvq_note_trainer_read.argtypes = [vp, C.c_int, fp, C.c_size_t]; L.pvq_note_trainer_read.restype = C.c_int
    L.pvq_note_trainer_dropout_keep.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, bp]
    L.pvq_note_trainer_dropout_keep.restype = C.c_int
    L.pvq_note_trainer_test.argtypes = [vp, vp, vp, C.c_size_t, up, C.c_size_t, C.c_uint32, C.POINTER(CNoteTestBatch), up, vp, vp]
    L.pvq_note_trainer_test.restype = C.c_int
    dp = C.POINTER(C.c_double)
    L.pvq_note_test_metrics.argtypes = [C.POINTER(CNoteTestBatch), C.c_size_t, dp, dp, dp]; L.pvq_note_test_metrics.restype = C.c_int
    if not _dev or _dev == "1" or hasattr(L, "pvq_note_trainer_epoch"):   # (as the carry above)
        L.pvq_note_trainer_epoch.argtypes = [vp, vp, vp, C.c_size_t, up, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, fp, dp, vp]
        L.pvq_note_trainer_epoch.restype = C.c_int
        L.pvq_note_epoch_order.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, up]; L.pvq_note_epoch_order.restype = C.c_int
        L.pvq_note_trainer_write.argtypes = [vp, C.c_int, fp, C.c_size_t]; L.pvq_note_trainer_write.restype = C.c_int
        L.pvq_note_trainer_set_steps.argtypes = [vp, C.c_uint64]; L.pvq_note_trainer_set_steps.restype = C.c_int
    L.pvq_host_alloc.argtypes = [C.c_size_t]; L.pvq_host_alloc.restype = C.c_void_p
    L.pvq_host_free.argtypes = [C.c_void_p]
    L.pvq_vqt_input_status.argtypes = [vp, vp]; L.pvq_vqt_input_status.restype = C.c_int
    L.pvq_vqt_last_gemm_flop.argtypes = [vp]; L.pvq_vqt_last_gemm_flop.restype = C.c_double
    L.pvq_vqt_last_sclk_mhz.argtypes = [vp]; L.pvq_vqt_last_sclk_mhz.restype = C.c_float
    _lib = L
    return L
