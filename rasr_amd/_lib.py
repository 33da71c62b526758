"""ctypes view of librasr_amd.so (include/amx.h).  No compute happens in Python.

The library is built in-tree by ``__graft_entry__.build()`` (``make -C rasr_amd/csrc``).  There is
no fallback: if the shared object is missing or no gfx950 device is visible, the calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMX_LIBRARY", os.path.join(_HERE, "librasr_amd.so"))  # AMX_LIBRARY: A/B runs of two builds (tools/)

AMX_OK, AMX_ERR_INVALID, AMX_ERR_UNSUPPORTED, AMX_ERR_DEVICE, AMX_ERR_STATE = 0, -1, -2, -3, -4
AMX_GMM_MAX, AMX_GMM_SUM, AMX_GMM_BATCH_FLOAT, AMX_GMM_SIMD, AMX_GMM_BATCH_INT, AMX_GMM_PRESELECTION_FLOAT, AMX_GMM_PRESELECTION_INT = 0, 1, 2, 3, 4, 5, 6
AMX_GMM_VITERBI, AMX_GMM_BAUM_WELCH = 0, 1
AMX_ACT_NONE, AMX_ACT_RELU, AMX_ACT_SIGMOID, AMX_ACT_TANH, AMX_ACT_ELU = 0, 1, 2, 3, 4
AMX_NN_PRE_LOGARITHM, AMX_NN_PRE_MEAN_AND_VARIANCE = 1, 2
AMX_NN_MAX_PRE = 4
AMX_PREC_FP32, AMX_PREC_BF16, AMX_PREC_BF16X3, AMX_PREC_F16MX = 0, 1, 2, 3
AMX_NN_TOP_LINEAR, AMX_NN_TOP_SOFTMAX = 0, 1
AMX_ARCHIVE_READ, AMX_ARCHIVE_WRITE = 0, 1
AMX_NORM_MEAN, AMX_NORM_MEAN_AND_VARIANCE = 0, 1


class AmxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("amx status %d: %s" % (status, message))
        self.status = status


class MfccCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("win_len_s", C.c_double), ("win_shift_s", C.c_double),
                ("preemph_alpha", C.c_double), ("fft_max_input_s", C.c_double), ("apply_scale", C.c_int),
                ("mel_filter_width", C.c_double), ("mel_spacing", C.c_double),
                ("warp_differential_unit", C.c_int), ("n_ceps", C.c_int), ("dct_normalize", C.c_int),
                ("front_end", C.c_int), ("n_autocorrelation", C.c_int), ("plp_power", C.c_double),
                ("filter_type", C.c_int), ("boundary", C.c_int), ("warping", C.c_int), ("tuning", C.c_char_p)]


class MfccVtln(C.Structure):
    _fields_ = [("limit", C.c_double), ("n_factors", C.c_int), ("factors", C.c_void_p)]


AMX_MFCC_MAX_WARPING_FACTORS = 64


class GammatoneCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("cascade", C.c_int), ("min_freq", C.c_double), ("max_freq", C.c_double), ("q", C.c_double),
                ("channels", C.c_int), ("cf_mode", C.c_int), ("warp_freq_break", C.c_double), ("warping_factor", C.c_double),
                ("ti_window", C.c_int), ("ti_length_s", C.c_double), ("ti_shift_s", C.c_double), ("si_window", C.c_int),
                ("si_length", C.c_int), ("si_shift", C.c_int), ("power", C.c_double), ("n_ceps", C.c_int), ("dct_normalize", C.c_int),
                ("tuning", C.c_char_p)]


class GammatoneInfo(C.Structure):
    _fields_ = [("channels", C.c_int), ("cascade", C.c_int), ("frame_len", C.c_int), ("frame_shift", C.c_int), ("si_channels", C.c_int),
                ("n_out", C.c_int)]


class VoicednessCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("win_len_s", C.c_double), ("win_shift_s", C.c_double), ("corr_begin_s", C.c_double),
                ("corr_end_s", C.c_double), ("normalization", C.c_int), ("min_position_s", C.c_double), ("max_position_s", C.c_double),
                ("tuning", C.c_char_p)]


class VoicednessInfo(C.Structure):
    _fields_ = [("frame_len", C.c_int), ("frame_shift", C.c_int), ("fft_len", C.c_int), ("n_lags", C.c_int), ("min_position", C.c_int),
                ("max_position", C.c_int)]


class HistogramInfo(C.Structure):
    _fields_ = [("dim", C.c_int), ("bucket_size", C.c_float), ("frozen", C.c_int), ("lds_max_buckets", C.c_int), ("lds_capacity", C.c_int),
                ("frames", C.c_ulonglong), ("n_lds", C.c_ulonglong), ("n_global", C.c_ulonglong), ("n_device_calls", C.c_ulonglong)]


class BayesCfg(C.Structure):
    _fields_ = [("n_classes", C.c_int), ("number_of_features", C.c_long), ("delay", C.c_long), ("window_length", C.c_int),
                ("window_right", C.c_int), ("single_frame", C.c_int)]


class PosteriorCfg(C.Structure):
    _fields_ = [("n_mixtures", C.c_int), ("scale", C.c_double), ("pruning_threshold", C.c_double), ("margin", C.c_double), ("viterbi", C.c_int)]


class PosteriorOut(C.Structure):
    _fields_ = [("posterior_f32_dev", C.c_void_p), ("posterior_f32_ld", C.c_int), ("posterior_f64_dev", C.c_void_p), ("posterior_f64_ld", C.c_int),
                ("log_z_dev", C.c_void_p), ("min_dev", C.c_void_p), ("min_index_dev", C.c_void_p), ("n_survivors_dev", C.c_void_p),
                ("sparse_index_dev", C.c_void_p), ("sparse_value_dev", C.c_void_p), ("sparse_count_dev", C.c_void_p), ("sparse_capacity", C.c_int)]


class AlignCfg(C.Structure):
    _fields_ = [("min_acoustic_pruning", C.c_float), ("max_acoustic_pruning", C.c_float), ("increment_factor", C.c_float),
                ("min_average_number_of_states", C.c_double), ("increase_until_no_score_difference", C.c_int), ("n_best_pruning", C.c_int),
                ("mode", C.c_int), ("score_scale", C.c_float)]


class AlignGraphs(C.Structure):
    _fields_ = [("state_offsets", C.c_void_p), ("initial_state", C.c_void_p), ("is_final", C.c_void_p), ("final_weight", C.c_void_p),
                ("arc_offsets", C.c_void_p), ("arc_target", C.c_void_p), ("arc_emission", C.c_void_p), ("arc_label", C.c_void_p),
                ("arc_weight", C.c_void_p)]


class AlignResult(C.Structure):
    _fields_ = [("score", C.c_float), ("reached_final", C.c_int), ("n_iterations", C.c_int), ("last_threshold", C.c_float),
                ("average_states", C.c_double), ("state_sum", C.c_ulonglong)]


class BwCfg(C.Structure):
    _fields_ = [("min_acoustic_pruning", C.c_float), ("max_acoustic_pruning", C.c_float), ("increment_factor", C.c_float),
                ("min_average_number_of_states", C.c_double), ("increase_until_no_score_difference", C.c_int), ("n_best_pruning", C.c_int),
                ("score_scale", C.c_float), ("min_weight", C.c_float), ("use_partial_sums", C.c_int)]


class BwResult(C.Structure):
    _fields_ = [("score", C.c_float), ("reached_final", C.c_int), ("n_iterations", C.c_int), ("last_threshold", C.c_float),
                ("average_states", C.c_double), ("state_sum", C.c_ulonglong), ("n_items", C.c_longlong), ("log_total", C.c_double)]


class LinsegCfg(C.Structure):
    _fields_ = [("number_of_iterations", C.c_int), ("penalty", C.c_double), ("minimum_speech_proportion", C.c_float), ("should_use_sietill", C.c_int),
                ("minimum_segment_length", C.c_int), ("maximum_segment_length", C.c_int)]


class LinsegResult(C.Structure):
    _fields_ = [("reason", C.c_int), ("speech_begin", C.c_int), ("speech_end", C.c_int), ("score", C.c_double)]


class LinsegModels(C.Structure):
    _fields_ = [("state_offsets", C.c_void_p), ("state_label", C.c_void_p), ("state_emission", C.c_void_p), ("silence_label", C.c_int),
                ("silence_emission", C.c_int)]


class CartProblem(C.Structure):
    _fields_ = [("n_examples", C.c_int), ("dim", C.c_int), ("n_questions", C.c_int), ("n_obs", C.c_void_p), ("values", C.c_void_p), ("answers", C.c_void_p)]


class CartStep(C.Structure):
    _fields_ = [("action", C.c_int), ("min_obs", C.c_uint), ("min_gain", C.c_double), ("randomize", C.c_int), ("n_questions", C.c_int),
                ("questions", C.c_void_p)]


class CartPlan(C.Structure):
    _fields_ = [("max_leaves", C.c_uint), ("n_steps", C.c_int), ("steps", C.c_void_p), ("variance_clipping", C.c_double), ("exact_all", C.c_int)]


class CartNode(C.Structure):
    _fields_ = [("step", C.c_int), ("row", C.c_int), ("left", C.c_int), ("right", C.c_int), ("depth", C.c_uint), ("n_obs", C.c_uint),
                ("score", C.c_double), ("class_id", C.c_int)]


class CartCommit(C.Structure):
    _fields_ = [("node", C.c_int), ("step", C.c_int), ("row", C.c_int), ("depth", C.c_uint), ("gain", C.c_double), ("total_gain", C.c_double)]


class CartQstat(C.Structure):
    _fields_ = [("step", C.c_int), ("row", C.c_int), ("count", C.c_uint), ("min_gain", C.c_double), ("sum_gain", C.c_double), ("max_gain", C.c_double),
                ("min_depth", C.c_uint), ("sum_depth", C.c_uint), ("max_depth", C.c_uint)]


class CartInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("n_leaves", C.c_int), ("n_commits", C.c_int), ("n_question_stats", C.c_int), ("n_examples", C.c_int),
                ("n_obs", C.c_uint), ("initial_score", C.c_double), ("total_gain", C.c_double), ("negative_gain_errors", C.c_ulonglong),
                ("items_screened", C.c_ulonglong), ("items_reevaluated", C.c_ulonglong), ("launches", C.c_ulonglong)]


AMX_CART_SPLIT, AMX_CART_PARTITION, AMX_CART_CLUSTER = range(3)


class CmllrShape(C.Structure):
    _fields_ = [("feature_dim", C.c_int), ("model_dim", C.c_int), ("n_keys", C.c_int), ("pooled", C.c_int)]


class MllrShape(C.Structure):
    _fields_ = [("mode", C.c_int), ("dim", C.c_int), ("n_leafs", C.c_int), ("n_keys", C.c_int)]


class EbwCfg(C.Structure):
    _fields_ = [("weight_threshold", C.c_float), ("viterbi", C.c_int)]


class EbwOffsets(C.Structure):
    _fields_ = [(n, C.c_long) for n in ("num_mixture_weights", "num_mean_weights", "num_mean_sums", "num_cov_weights", "num_cov_sums",
                                        "den_density_weights", "den_mean_weights", "den_mean_sums", "den_cov_weights", "den_cov_sums",
                                        "objective", "size", "n_slots", "n_means", "n_covariances", "dim")]


class EbwCallShape(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("item_sort_passes", "list_sort_passes", "item_blocks", "list_blocks", "item_table_recursed",
                                       "list_table_recursed")]


class LatpostCfg(C.Structure):
    _fields_ = [("mode", C.c_int), ("normalize", C.c_int), ("v_normalized", C.c_int), ("tolerance", C.c_int), ("potentials", C.c_int)]


class LatpostInfo(C.Structure):
    _fields_ = [("total_inv", C.c_double), ("total_inv_f32", C.c_float), ("expectation", C.c_float), ("forward_flow", C.c_float),
                ("backward_flow", C.c_float)] + \
        [(n, C.c_int) for n in ("flows_agree", "vanishing_flow", "reason", "states_reached", "arcs_reached", "states_coreached",
                                "undefined_states", "undefined_arcs", "levels_forward", "levels_backward")]


class NnSeqCfg(C.Structure):
    _fields_ = [("weight_threshold", C.c_double), ("ce_smoothing_weight", C.c_float), ("frame_rejection_threshold", C.c_float),
                ("log_prior", C.c_void_p), ("prior_scale", C.c_float), ("full_batch", C.c_int), ("accumulate_prior", C.c_int),
                ("label_type", C.c_int), ("keep_lattice_error", C.c_int)]


class NnSeqPass(C.Structure):
    _fields_ = [("arc_offsets", C.c_void_p), ("item_offsets", C.c_void_p), ("item_frame", C.c_void_p), ("item_emission", C.c_void_p),
                ("arc_weight_dev", C.c_void_p), ("negate", C.c_int), ("factor", C.c_double), ("role", C.c_int)]


class NnSeqInfo(C.Structure):
    _fields_ = [("segments_processed", C.c_int), ("segments_skipped", C.c_int), ("segments_without_alignment", C.c_int),
                ("observations", C.c_long), ("rejected_observations", C.c_long), ("ce_objective", C.c_float),
                ("seg_reason", C.c_void_p), ("seg_errors", C.c_void_p), ("seg_rejected", C.c_void_p), ("seg_ce_objective", C.c_void_p)]


class EbwEstimateCfg(C.Structure):
    _fields_ = [("min_observation_weight", C.c_double), ("min_relative_weight", C.c_double), ("min_variance", C.c_double),
                ("normalize_mixture_weights", C.c_int), ("iteration_constants", C.c_int), ("step_size", C.c_double), ("minimum_icd", C.c_double),
                ("beta", C.c_double), ("sigma_minimum", C.c_double), ("sigma_minimum_factor", C.c_double), ("number_of_iterations", C.c_int),
                ("i_smoothing_means", C.c_double), ("i_smoothing_weights", C.c_double), ("viterbi", C.c_int), ("estimator", C.c_int),
                ("contract", C.c_int)]


class EbwEstimateInfo(C.Structure):
    _fields_ = [("i_smoothing_objective", C.c_double), ("sigma_minimum", C.c_double), ("n_removed", C.c_int), ("n_clamped", C.c_int),
                ("n_mean_fallback", C.c_int), ("n_floored", C.c_int)]


class MllrTree(C.Structure):
    _fields_ = [("n_ids", C.c_int), ("root", C.c_int), ("left", C.c_void_p), ("right", C.c_void_p), ("previous", C.c_void_p),
                ("leaf_number", C.c_void_p), ("n_leaf_list", C.c_int), ("leaf_list", C.c_void_p), ("n_silence", C.c_int),
                ("silence_mixtures", C.c_void_p)]
(AMX_LINSEG_OK, AMX_LINSEG_TOO_SHORT, AMX_LINSEG_TOO_LONG, AMX_LINSEG_NO_STATES, AMX_LINSEG_JUMP, AMX_LINSEG_MISMATCH, AMX_LINSEG_NONFINITE,
 AMX_LINSEG_N_REASONS) = range(8)
AMX_BW_MAX_LABELS = 4096
AMX_ALIGN_MAX_STATES, AMX_ALIGN_MAX_EMISSIONS, AMX_ALIGN_MAX_OUT_ARCS, AMX_ALIGN_MAX_PASSES = 2048, 4096, 64, 4096
AMX_ALIGN_VITERBI, AMX_ALIGN_BAUM_WELCH = 0, 1
AMX_POSTERIOR_MIXTURE, AMX_POSTERIOR_LIKELIHOOD, AMX_POSTERIOR_DENSITY = 0, 1, 2
AMX_COMBINE_MAX_MODELS = 8


class QuanteqCfg(C.Structure):
    _fields_ = [("quantiles", C.c_int), ("combination", C.c_int), ("estimate", C.c_int), ("mean", C.c_int), ("variance", C.c_int),
                ("number_of_quantiles", C.c_int), ("overestimation_factor", C.c_float), ("delta_alpha", C.c_float), ("delta_gamma", C.c_float),
                ("delta_lambda_and_rho", C.c_float), ("beta", C.c_float), ("pool_quantiles", C.c_int), ("piecewise_linear", C.c_int),
                ("length", C.c_long), ("right", C.c_long)]


AMX_QUANTEQ_MAX_DIM, AMX_QUANTEQ_MAX_QUANTILES, AMX_QUANTEQ_MAX_GRID_SIDE, AMX_QUANTEQ_MAX_SEGMENT_FRAMES = 4096, 16, 4096, 16384
AMX_XCORR_NONE, AMX_XCORR_UNBIASED_ESTIMATE, AMX_XCORR_UPPER_BOUND = 0, 1, 2


class MfccInfo(C.Structure):
    _fields_ = [("frame_len", C.c_int), ("frame_shift", C.c_int), ("fft_len", C.c_int), ("n_bins", C.c_int),
                ("n_filters", C.c_int), ("n_ceps", C.c_int), ("fft_output_sample_rate", C.c_double),
                ("mel_max", C.c_double), ("n_transform", C.c_int), ("n_transform_inputs", C.c_int)]


class GmmModel(C.Structure):
    _fields_ = [("dim", C.c_int), ("n_mix", C.c_int), ("n_dens", C.c_int), ("n_mean", C.c_int), ("n_cov", C.c_int),
                ("mix_offsets", C.c_void_p), ("dens_index", C.c_void_p), ("log_weight", C.c_void_p),
                ("dens_mean", C.c_void_p), ("dens_cov", C.c_void_p), ("means", C.c_void_p),
                ("variances", C.c_void_p), ("mixture_weight_scale", C.c_double), ("gaussian_scale", C.c_double), ("tuning", C.c_char_p)]


class GmmEstimateCfg(C.Structure):
    _fields_ = [("min_observation_weight", C.c_double), ("min_relative_weight", C.c_double), ("min_variance", C.c_double),
                ("normalize_mixture_weights", C.c_int), ("allow_zero_weights", C.c_int), ("split", C.c_int),
                ("split_min_mean_observation_weight", C.c_double), ("split_min_covariance_observation_weight", C.c_double),
                ("split_perturbation_weight", C.c_double), ("split_normalize_mixture_weights", C.c_int)]


class FfnnModel(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("in_dim", C.c_void_p), ("out_dim", C.c_void_p), ("W", C.c_void_p),
                ("bias", C.c_void_p), ("activation", C.c_void_p), ("log_prior", C.c_void_p),
                ("prior_scale", C.c_float), ("precision", C.c_int), ("n_classes", C.c_int), ("class_to_output", C.c_void_p),
                ("tuning", C.c_char_p)]


class FfnnLayers(C.Structure):
    _fields_ = [("n_pre", C.c_int), ("pre_type", C.c_void_p), ("pre_mean", C.c_void_p), ("pre_stddev", C.c_void_p),
                ("maxout_groups", C.c_void_p), ("maxout_sizes", C.c_void_p)]


AMX_NNSTAT_CLASS_COUNTS, AMX_NNSTAT_MEAN_AND_VARIANCE, AMX_NNSTAT_BASE, AMX_NNSTAT_GRADIENT = 1, 2, 4, 8
AMX_NNTRAIN_CHUNK, AMX_NNTRAIN_MAX_FRAMES, AMX_NNTRAIN_MAX_LAYERS = 256, 4096, 16


class NnTrainCfg(C.Structure):
    _fields_ = [("statistics", C.c_int), ("error_signal_clip", C.c_float), ("class_weights", C.c_void_p), ("feature_dim", C.c_int),
                ("n_outputs", C.c_int), ("n_classes", C.c_int), ("class_to_output", C.c_void_p)]


class NnTrainLayout(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("feature_dim", C.c_int), ("n_outputs", C.c_int),
                ("in_dim", C.c_int * AMX_NNTRAIN_MAX_LAYERS), ("out_dim", C.c_int * AMX_NNTRAIN_MAX_LAYERS),
                ("gradient_weights", C.c_long * AMX_NNTRAIN_MAX_LAYERS), ("gradient_bias", C.c_long * AMX_NNTRAIN_MAX_LAYERS),
                ("feature_sum", C.c_long), ("feature_square_sum", C.c_long), ("class_counts", C.c_long), ("tail", C.c_long), ("size", C.c_long)]


AMX_NNSTEP_REG_NONE, AMX_NNSTEP_REG_L1, AMX_NNSTEP_REG_L2, AMX_NNSTEP_REG_CENTERED_L2 = 0, 1, 2, 3
AMX_NNSTEP_MEAN_NORMALIZED_SGD, AMX_NNSTEP_MEAN_NORMALIZED_SGD_L1_CLIPPING = 0, 1
AMX_NNSTEP_STAT_NO_STATISTICS, AMX_NNSTEP_STAT_NONE, AMX_NNSTEP_STAT_EXPONENTIAL_TRACE = 0, 1, 2


class NnStepCfg(C.Structure):
    _fields_ = [("learning_rate", C.c_float), ("bias_learning_rate", C.c_float), ("layer_learning_rate", C.c_void_p),
                ("regularization_constant", C.c_void_p), ("trainable", C.c_void_p), ("regularizer", C.c_int), ("center_W", C.c_void_p),
                ("center_bias", C.c_void_p), ("center_in_dim", C.c_void_p), ("center_out_dim", C.c_void_p), ("estimator", C.c_int),
                ("accumulate_multiple_batches", C.c_int), ("normalize_by_observations", C.c_int), ("log_step_size", C.c_int),
                ("update_input_layer_weights", C.c_int), ("statistics_smoothing", C.c_void_p), ("trace_factor", C.c_void_p),
                ("initial_activation_mean", C.c_void_p), ("initial_activation_stddev", C.c_void_p), ("input_smoothing", C.c_int),
                ("input_trace_factor", C.c_float), ("input_initial_mean", C.c_void_p), ("input_initial_stddev", C.c_void_p)]


class NnStepInfo(C.Structure):
    _fields_ = [("minibatch", C.c_long), ("updated", C.c_int), ("n_observations", C.c_long), ("n_classification_errors", C.c_long),
                ("total_weight", C.c_float), ("objective", C.c_float), ("criterion_objective", C.c_float),
                ("step_size", C.c_float * AMX_NNTRAIN_MAX_LAYERS)]


# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against amx.h
_P = C.c_void_p
SIGNATURES = {
    "amx_version": (C.c_char_p, []),
    "amx_last_error": (C.c_char_p, []),
    "amx_init": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "amx_destroy": (None, [_P]),
    "amx_set_stream": (C.c_int, [_P, _P]),
    "amx_set_contract": (C.c_int, [_P, C.c_int]),
    "amx_get_contract": (C.c_int, [_P]),
    "amx_contract_description": (C.c_char_p, [C.c_int]),
    "amx_synchronize": (C.c_int, [_P]),
    "amx_profile_enable": (C.c_int, [_P, C.c_int]),
    "amx_profile_reset": (C.c_int, [_P]),
    "amx_profile_get": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "amx_mfcc_default_cfg": (None, [C.POINTER(MfccCfg)]),
    "amx_mfplp_default_cfg": (None, [C.POINTER(MfccCfg)]),
    "amx_plp_default_cfg": (None, [C.POINTER(MfccCfg)]),
    "amx_gammatone_default_cfg": (None, [C.POINTER(GammatoneCfg)]),
    "amx_gammatone_create": (C.c_int, [_P, C.POINTER(GammatoneCfg), C.POINTER(C.c_void_p)]),
    "amx_gammatone_destroy": (None, [_P]),
    "amx_gammatone_describe": (C.c_int, [_P, C.POINTER(GammatoneInfo)]),
    "amx_gammatone_n_frames": (C.c_long, [_P, C.c_long]),
    "amx_gammatone_tables": (C.c_int, [_P, _P, _P]),
    "amx_gammatone_run": (C.c_int, [_P, _P, C.c_long, _P]),
    "amx_gammatone_run_batch_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "amx_voicedness_default_cfg": (None, [C.POINTER(VoicednessCfg)]),
    "amx_voicedness_create": (C.c_int, [_P, C.POINTER(VoicednessCfg), C.POINTER(C.c_void_p)]),
    "amx_voicedness_destroy": (None, [_P]),
    "amx_voicedness_describe": (C.c_int, [_P, C.POINTER(VoicednessInfo)]),
    "amx_voicedness_n_frames": (C.c_long, [_P, C.c_long]),
    "amx_voicedness_run": (C.c_int, [_P, _P, C.c_long, _P]),
    "amx_voicedness_run_batch_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "amx_voicedness_run_batch_dev_s16": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "amx_voicedness_energy_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "amx_mfcc_equal_loudness": (C.c_int, [_P, _P]),
    "amx_mfcc_create": (C.c_int, [_P, C.POINTER(MfccCfg), C.POINTER(_P)]),
    "amx_mfcc_destroy": (None, [_P]),
    "amx_mfcc_describe": (C.c_int, [_P, C.POINTER(MfccInfo)]),
    "amx_mfcc_n_frames": (C.c_long, [_P, C.c_long]),
    "amx_mfcc_frame_start_time": (C.c_double, [_P, C.c_long]),
    "amx_mfcc_tables": (C.c_int, [_P] * 7),
    "amx_mfcc_run": (C.c_int, [_P, _P, C.c_long, _P]),
    "amx_mfcc_run_batch": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "amx_mfcc_run_s16": (C.c_int, [_P, _P, C.c_long, _P]),
    "amx_mfcc_run_batch_s16": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "amx_mfcc_plan_create": (C.c_int, [_P, C.c_int, _P, C.POINTER(_P)]),
    "amx_mfcc_plan_destroy": (None, [_P]),
    "amx_mfcc_plan_total_frames": (C.c_long, [_P]),
    "amx_mfcc_plan_frame_offsets": (C.c_int, [_P, _P]),
    "amx_mfcc_run_plan_dev": (C.c_int, [_P, _P, _P, _P]),
    "amx_mfcc_run_plan_dev_s16": (C.c_int, [_P, _P, _P, _P]),
    "amx_mfcc_create_vtln": (C.c_int, [_P, C.POINTER(MfccCfg), C.POINTER(MfccVtln), C.POINTER(_P)]),
    "amx_mfcc_plan_create_vtln": (C.c_int, [_P, C.c_int, _P, _P, C.POINTER(_P)]),
    "amx_mfcc_tables_vtln": (C.c_int, [_P, C.c_double] + [_P] * 6),
    "amx_context_window_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "amx_normalize_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "amx_normalize_ex_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "amx_vector_normalize_dev": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_long, C.c_int, _P, C.c_int]),
    "amx_vector_function_dev": (C.c_int, [_P, C.c_int, C.c_float, _P, C.c_int, C.c_long, C.c_int, _P, C.c_int]),
    "amx_regression_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "amx_matrix_multiply_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int]),
    "amx_gmm_create": (C.c_int, [_P, C.POINTER(GmmModel), C.POINTER(_P)]),
    "amx_gmm_destroy": (None, [_P]),
    "amx_gmm_n_mixtures": (C.c_int, [_P]),
    "amx_gmm_dimension": (C.c_int, [_P]),
    "amx_gmm_tables": (C.c_int, [_P, _P, _P, _P]),
    "amx_gmm_simd_scaling": (C.c_float, [_P]),
    "amx_gmm_set_preselection": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float]),
    "amx_gmm_preselection_clustering": (C.c_int, [_P, C.POINTER(C.c_int), _P, _P]),
    "amx_gmm_preselection_int_clustering": (C.c_int, [_P, C.POINTER(C.c_int), _P, _P]),
    "amx_gmm_screen_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "amx_gmm_score": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "amx_gmm_score_dev": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "amx_gmm_score_stats_dev": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "amx_gmm_score_stats_u8_dev": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "amx_gmm_best_density_dev": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "amx_gmm_accumulator_size": (C.c_long, [_P]),
    "amx_gmm_accumulate_u8_dev": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "amx_gmm_accumulate_dev": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "amx_gmm_accumulate_weighted_dev": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "amx_scatter_accumulator_size": (C.c_long, [C.c_int, C.c_int]),
    "amx_scatter_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_long, C.c_int, _P, C.c_int, _P, _P]),
    "amx_scatter_accumulator_write": (C.c_int, [C.c_int, C.c_int, _P, C.c_char_p]),
    "amx_scatter_accumulator_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_scatter_finalize": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "amx_matrix_read_f64": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_matrix_write_f64": (C.c_int, [C.c_char_p, C.c_int, C.c_int, _P]),
    "amx_histogram_create": (C.c_int, [_P, C.c_int, C.c_float, C.POINTER(_P)]),
    "amx_histogram_destroy": (None, [_P]),
    "amx_histogram_attach": (C.c_int, [_P, _P]),
    "amx_histogram_describe": (C.c_int, [_P, C.POINTER(HistogramInfo)]),
    "amx_histogram_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_long]),
    "amx_histogram_accumulate": (C.c_int, [_P, _P, C.c_int, C.c_long]),
    "amx_histogram_write": (C.c_int, [_P, C.c_char_p]),
    "amx_histogram_read": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "amx_histogram_table": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "amx_histogram_cdf": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "amx_histogram_percentile": (C.c_int, [_P, C.c_int, C.c_float, C.POINTER(C.c_float)]),
    "amx_histnorm_create": (C.c_int, [_P, C.c_int, _P, C.c_float, C.POINTER(_P)]),
    "amx_histnorm_destroy": (None, [_P]),
    "amx_histnorm_set_scales": (C.c_int, [_P, _P]),
    "amx_histnorm_add_key": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "amx_histnorm_n_keys": (C.c_int, [_P]),
    "amx_histnorm_inverse_cdf": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "amx_histnorm_test_cdf": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "amx_histnorm_apply_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, C.c_int, _P]),
    "amx_bayes_default_cfg": (None, [C.POINTER(BayesCfg)]),
    "amx_bayes_create": (C.c_int, [_P, C.POINTER(BayesCfg), C.POINTER(_P)]),
    "amx_bayes_destroy": (None, [_P]),
    "amx_bayes_prior": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "amx_bayes_classify_dev": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "amx_bayes_scores_dev": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "amx_bayes_classify_gmm_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "amx_gmm_topology": (C.c_int, [_P, C.POINTER(C.c_int), _P, _P]),
    "amx_posterior_default_cfg": (None, [C.POINTER(PosteriorCfg)]),
    "amx_posterior_create": (C.c_int, [_P, C.POINTER(PosteriorCfg), C.POINTER(_P)]),
    "amx_posterior_destroy": (None, [_P]),
    "amx_posterior_set_filter": (C.c_int, [_P, C.c_int, _P, _P]),
    "amx_posterior_set_default_filter": (C.c_int, [_P]),
    "amx_posterior_set_single_filter": (C.c_int, [_P, C.c_int]),
    "amx_posterior_set_disregard": (C.c_int, [_P, C.c_int, _P]),
    "amx_posterior_filter": (C.c_int, [_P, C.POINTER(C.c_int), _P, _P]),
    "amx_posterior_set_topology": (C.c_int, [_P, _P, _P]),
    "amx_posterior_set_topology_gmm": (C.c_int, [_P, _P]),
    "amx_posterior_topology_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "amx_posterior_dev": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.POINTER(PosteriorOut), _P]),
    "amx_posterior_lists_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "amx_posterior_gmm_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.POINTER(PosteriorOut), _P]),
    "amx_combine_create": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(_P)]),
    "amx_combine_destroy": (None, [_P]),
    "amx_combine_identity_columns": (C.c_int, [_P, C.POINTER(C.c_uint)]),
    "amx_combine_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "amx_align_default_cfg": (None, [C.POINTER(AlignCfg)]),
    "amx_align_create": (C.c_int, [_P, C.POINTER(AlignCfg), C.POINTER(_P)]),
    "amx_align_destroy": (None, [_P]),
    "amx_align_viterbi_dev": (C.c_int, [_P, C.c_int, _P, C.POINTER(AlignGraphs), _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "amx_bw_default_cfg": (None, [C.POINTER(BwCfg)]),
    "amx_bw_create": (C.c_int, [_P, C.POINTER(BwCfg), C.POINTER(_P)]),
    "amx_bw_destroy": (None, [_P]),
    "amx_bw_n_items": (C.c_longlong, [_P]),
    "amx_bw_align_dev": (C.c_int, [_P, C.c_int, _P, C.POINTER(AlignGraphs), _P, C.c_int, C.c_int, _P, _P, _P]),
    "amx_bw_items_dev": (C.c_int, [_P, C.c_longlong, _P, _P, _P, _P, _P]),
    "amx_gather_rows_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_longlong, _P, _P, C.c_int]),
    "amx_linseg_default_cfg": (None, [C.POINTER(LinsegCfg)]),
    "amx_linseg_create": (C.c_int, [_P, C.POINTER(LinsegCfg), C.POINTER(_P)]),
    "amx_linseg_destroy": (None, [_P]),
    "amx_linseg_align_dev": (C.c_int, [_P, C.c_int, _P, C.POINTER(LinsegModels), _P, C.c_int, _P, _P, _P, _P]),
    "amx_linseg_chains": (C.c_int, [_P, C.c_int, _P, _P]),
    "amx_cart_accumulator_size": (C.c_size_t, [C.c_int, C.c_int]),
    "amx_cart_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    "amx_cart_train": (C.c_int, [_P, C.POINTER(CartProblem), C.POINTER(CartPlan), C.POINTER(_P)]),
    "amx_cart_tree_destroy": (None, [_P]),
    "amx_cart_tree_info": (C.c_int, [_P, C.POINTER(CartInfo)]),
    "amx_cart_tree_get": (C.c_int, [_P, _P, _P, _P, _P]),
    "amx_cart_kernel_shape": (None, [C.c_int, _P, _P]),
    "amx_quanteq_default_cfg": (None, [C.POINTER(QuanteqCfg)]),
    "amx_quanteq_create": (C.c_int, [_P, C.c_int, C.POINTER(QuanteqCfg), _P, C.POINTER(_P)]),
    "amx_quanteq_destroy": (None, [_P]),
    "amx_quanteq_grid": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), _P]),
    "amx_quanteq_quantiles_read": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, _P]),
    "amx_quanteq_quantiles_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, _P, C.c_ulonglong]),
    "amx_quanteq_apply_dev": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P]),
    "amx_quanteq_estimate_dev": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "amx_quanteq_estimate_result": (C.c_int, [_P, _P, C.POINTER(C.c_ulonglong)]),
    "amx_gmm_estimate_cfg_default": (None, [C.POINTER(GmmEstimateCfg)]),
    "amx_gmm_estimate": (C.c_int, [C.POINTER(GmmModel), _P, C.POINTER(GmmEstimateCfg), C.POINTER(_P)]),
    "amx_gmm_accumulator_write": (C.c_int, [_P, _P, C.c_char_p]),
    "amx_gmm_accumulator_read": (C.c_int, [_P, C.c_char_p, _P]),
    "amx_pms_read": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "amx_pms_write": (C.c_int, [C.POINTER(GmmModel), C.c_char_p]),
    "amx_mixture_set_view": (C.c_int, [_P, C.POINTER(GmmModel)]),
    "amx_mixture_set_destroy": (None, [_P]),
    "amx_ffnn_create": (C.c_int, [_P, C.POINTER(FfnnModel), C.POINTER(_P)]),
    "amx_ffnn_create_ex": (C.c_int, [_P, C.POINTER(FfnnModel), C.POINTER(FfnnLayers), C.POINTER(_P)]),
    "amx_ffnn_destroy": (None, [_P]),
    "amx_ffnn_input_dim": (C.c_int, [_P]),
    "amx_ffnn_output_dim": (C.c_int, [_P]),
    "amx_ffnn_score": (C.c_int, [_P, _P, C.c_int, _P]),
    "amx_ffnn_score_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "amx_device_clocks_dev": (C.c_int, [_P, _P]),
    "amx_device_clocks_xcd_dev": (C.c_int, [_P, _P]),
    "amx_ffnn_wait_dev": (C.c_int, [_P]),
    "amx_ffnn_precision": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "amx_ffnn_score_stats_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "amx_ffnn_hidden_dim": (C.c_int, [_P]),
    "amx_dc_detection": (C.c_int, [_P, C.c_longlong, C.c_double, C.c_double, C.c_float, C.c_double, C.c_int, C.c_int, _P, _P, C.c_longlong, _P]),
    "amx_ffnn_forward_hidden_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "amx_ffnn_forward_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "amx_ffnn_score_on_demand_dev": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "amx_precomputed_score_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_float, _P]),
    "amx_class_labels_init": (C.c_int, [C.c_int, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "amx_nn_vector_read_f32": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_nn_vector_write_f32": (C.c_int, [C.c_char_p, C.c_int, _P]),
    "amx_nn_vector_read_s32": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_nn_vector_write_s32": (C.c_int, [C.c_char_p, C.c_int, _P]),
    "amx_nn_vector_read_u32": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_nn_matrix_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_nn_matrix_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, _P]),
    "amx_free": (None, [_P]),
    "amx_nn_layer_from_parameters": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "amx_prior_from_mixture_set": (C.c_int, [C.POINTER(GmmModel), _P]),
    "amx_archive_open": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "amx_archive_close": (C.c_int, [_P]),
    "amx_archive_n_files": (C.c_int, [_P]),
    "amx_archive_file_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "amx_archive_has_file": (C.c_int, [_P, C.c_char_p]),
    "amx_archive_read_file": (C.c_int, [_P, C.c_char_p, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "amx_archive_write_file": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t, C.c_int]),
    "amx_archive_remove_file": (C.c_int, [_P, C.c_char_p]),
    "amx_feature_cache_write": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, _P, _P, C.c_uint, C.c_int]),
    "amx_feature_cache_read": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P), C.POINTER(_P)]),
    "amx_feature_cache_write_attributes": (C.c_int, [_P, C.c_char_p, C.c_int, _P, _P, C.c_int]),
    "amx_feature_cache_read_attributes": (C.c_int, [_P, C.c_char_p, C.POINTER(_P)]),
    "amx_device_malloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "amx_device_free": (None, [_P, _P]),
    "amx_copy_to_device": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "amx_copy_to_host": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "amx_gather_scores": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "amx_stats_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "amx_comm_available": (C.c_int, []),
    "amx_comm_unique_id": (C.c_int, [_P]),
    "amx_comm_init": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "amx_comm_rank": (C.c_int, [_P]),
    "amx_comm_world": (C.c_int, [_P]),
    "amx_comm_all_reduce_f64_dev": (C.c_int, [_P, _P, C.c_size_t]),
    "amx_comm_destroy": (None, [_P]),
    "amx_counts_to_f64_dev": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "amx_f64_to_counts_dev": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "amx_nntrain_default_cfg": (None, [C.POINTER(NnTrainCfg)]),
    "amx_nntrain_create": (C.c_int, [_P, C.POINTER(FfnnModel), C.POINTER(FfnnLayers), C.POINTER(NnTrainCfg), C.POINTER(_P)]),
    "amx_nntrain_destroy": (None, [_P]),
    "amx_nntrain_accumulator_size": (C.c_long, [_P]),
    "amx_nntrain_layout": (C.c_int, [_P, C.POINTER(NnTrainLayout)]),
    "amx_nntrain_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "amx_nnstat_write": (C.c_int, [_P, _P, C.c_char_p]),
    "amx_nnstat_read": (C.c_int, [_P, C.c_char_p, _P]),
    "amx_nnstat_combine": (C.c_int, [_P, C.POINTER(C.c_char_p), C.c_int, _P]),
    "amx_prior_from_class_counts": (C.c_int, [_P, _P, C.c_float, _P]),
    "amx_nnstat_mean_and_deviation": (C.c_int, [_P, _P, _P, _P]),
    "amx_nnstep_default_cfg": (None, [C.POINTER(NnStepCfg)]),
    "amx_nntrain_set_estimator": (C.c_int, [_P, C.POINTER(NnStepCfg)]),
    "amx_nntrain_step_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "amx_nntrain_step_estimate_dev": (C.c_int, [_P]),
    "amx_nntrain_step_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(NnStepInfo)]),
    "amx_nntrain_step_info": (C.c_int, [_P, C.POINTER(NnStepInfo)]),
    "amx_nntrain_estimate": (C.c_int, [_P, _P, C.POINTER(NnStepInfo)]),
    "amx_nntrain_get_parameters": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "amx_nntrain_get_step_statistics": (C.c_int, [_P, C.c_int, _P, _P]),
    "amx_nntrain_get_activation_statistics": (C.c_int, [_P, C.c_int, _P, _P]),
    "amx_nntrain_get_layer_input": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "amx_cmllr_create": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "amx_cmllr_destroy": (None, [_P]),
    "amx_cmllr_describe": (C.c_int, [_P, C.POINTER(CmllrShape), _P]),
    "amx_cmllr_accumulator_size": (C.c_long, [_P]),
    "amx_cmllr_key_size": (C.c_long, [C.POINTER(CmllrShape)]),
    "amx_cmllr_kernel_shape": (None, [_P, _P, _P]),
    "amx_cmllr_set_tile": (C.c_int, [_P, C.c_int]),
    "amx_cmllr_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P]),
    "amx_cmllr_apply_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P]),
    "amx_cmllr_accumulator_write": (C.c_int, [C.POINTER(CmllrShape), _P, _P, C.c_char_p]),
    "amx_cmllr_accumulator_read": (C.c_int, [C.POINTER(CmllrShape), _P, C.c_char_p, _P]),
    "amx_cmllr_combine": (C.c_int, [C.POINTER(CmllrShape), _P, _P, C.POINTER(CmllrShape), _P, _P, C.c_double]),
    "amx_cmllr_estimate": (C.c_int, [C.POINTER(CmllrShape), _P, _P, C.c_int, C.c_double, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    "amx_cmllr_score": (C.c_int, [C.POINTER(CmllrShape), _P, _P, _P, C.c_int, _P]),
    "amx_cmllr_transform_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, _P]),
    "amx_cmllr_transform_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P)]),
    "amx_mllr_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "amx_mllr_destroy": (None, [_P]),
    "amx_mllr_describe": (C.c_int, [_P, C.POINTER(MllrShape)]),
    "amx_mllr_accumulator_size": (C.c_long, [_P]),
    "amx_mllr_leaf_size": (C.c_long, [C.POINTER(MllrShape)]),
    "amx_mllr_key_size": (C.c_long, [C.POINTER(MllrShape)]),
    "amx_mllr_kernel_shape": (None, [_P, _P]),
    "amx_mllr_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P]),
    "amx_mllr_adapt_means_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "amx_mllr_accumulator_write": (C.c_int, [C.POINTER(MllrShape), _P, C.c_char_p, C.c_double, C.c_double, C.c_int, _P, C.c_int, _P, C.c_char_p]),
    "amx_mllr_accumulator_read": (C.c_int, [C.POINTER(MllrShape), C.c_char_p, _P, _P, _P]),
    "amx_mllr_estimate": (C.c_int, [C.POINTER(MllrShape), _P, C.POINTER(MllrTree), C.c_int, _P, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P,
                                    _P, _P]),
    "amx_mllr_adaptor_write": (C.c_int, [C.POINTER(MllrShape), C.c_char_p, C.c_int, _P, _P, C.c_int, _P, C.c_char_p]),
    "amx_mllr_adaptor_read": (C.c_int, [C.POINTER(MllrShape), C.c_char_p, C.c_int, _P, _P, _P, C.c_int, _P]),
    "amx_ebw_cfg_default": (None, [C.POINTER(EbwCfg)]),
    "amx_ebw_create": (C.c_int, [_P, C.POINTER(EbwCfg), C.POINTER(_P)]),
    "amx_ebw_destroy": (None, [_P]),
    "amx_ebw_accumulator_size": (C.c_long, [_P]),
    "amx_ebw_layout": (C.c_int, [_P, C.POINTER(EbwOffsets)]),
    "amx_ebw_accumulate_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "amx_ebw_accumulate_objective": (C.c_int, [_P, C.c_float, _P]),
    "amx_ebw_last_keys": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), _P, _P, _P, _P, _P]),
    "amx_ebw_kernel_shape": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "amx_ebw_last_shape": (C.c_int, [_P, C.POINTER(EbwCallShape)]),
    "amx_ebw_topology_accumulator_size": (C.c_long, [_P]),
    "amx_ebw_accumulator_write": (C.c_int, [_P, _P, C.c_char_p]),
    "amx_ebw_accumulator_read": (C.c_int, [_P, C.c_char_p, _P]),
    "amx_ebw_accumulator_combine": (C.c_int, [_P, _P, _P]),
    "amx_ebw_estimate_cfg_default": (None, [C.POINTER(EbwEstimateCfg)]),
    "amx_ebw_estimate": (C.c_int, [_P, _P, _P, _P, C.POINTER(EbwEstimateCfg), C.POINTER(_P), C.POINTER(EbwEstimateInfo), _P]),
    "amx_latpost_cfg_default": (None, [C.POINTER(LatpostCfg)]),
    "amx_latpost_create": (C.c_int, [_P, C.POINTER(LatpostCfg), C.POINTER(_P)]),
    "amx_latpost_destroy": (None, [_P]),
    "amx_latpost_kernel_shape": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "amx_latpost_run_dev": (C.c_int, [_P, C.c_int] + [_P] * 12),
    "amx_latpost_plan_host": (C.c_int, [_P, C.c_int] + [_P] * 17),
    "amx_latpost_last_potentials": (C.c_int, [_P, C.c_long, _P, _P, _P, _P]),
    "amx_latpost_last_timing": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "amx_nnseq_default_cfg": (None, [C.POINTER(NnSeqCfg)]),
    "amx_nnseq_create": (C.c_int, [_P, C.POINTER(NnSeqCfg), C.POINTER(_P)]),
    "amx_nnseq_destroy": (None, [_P]),
    "amx_nnseq_forward_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "amx_nnseq_arc_scores_dev": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "amx_nnseq_accumulate_dev": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.POINTER(NnSeqInfo)]),
    "amx_nnseq_workspace_row": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "amx_nnseq_get_top": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "amx_nnseq_get_error_signal": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "amx_nnseq_get_weights": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "amx_nnseq_kernel_shape": (None, [C.POINTER(C.c_int)] * 4),
    "amx_nnseq_last_shape": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}
AMX_NNSEQ_ADD, AMX_NNSEQ_ADD_REJECT, AMX_NNSEQ_ADD_REJECT_CLEAR = 0, 1, 2
AMX_NNSEQ_SEG_OK, AMX_NNSEQ_SEG_SKIPPED, AMX_NNSEQ_SEG_NO_ALIGNMENT = 0, 1, 2
AMX_CMLLR_NAIVE, AMX_CMLLR_MMI_PRIME, AMX_CMLLR_HLDA = 0, 1, 2
AMX_MLLR_FULL, AMX_MLLR_SHIFT, AMX_MLLR_BAND, AMX_MLLR_SEMI_TIED = 0, 1, 2, 3
AMX_EBW_IC_GLOBAL_RWTH, AMX_EBW_IC_LOCAL_RWTH, AMX_EBW_IC_CAMBRIDGE = 0, 1, 2
AMX_EBW_ESTIMATOR_EBW, AMX_EBW_ESTIMATOR_RPROP = 0, 1
AMX_LATPOST_LOG, AMX_LATPOST_PROB, AMX_LATPOST_EXPECTATION = 0, 1, 2
AMX_LATPOST_OK, AMX_LATPOST_NO_FINAL = 0, 1
AMX_LATPOST_POTENTIALS_AUTO, AMX_LATPOST_POTENTIALS_GLOBAL = 0, 1
AMX_MLLR_ROOT_FALLBACK, AMX_MLLR_SILENCE_FALLBACK = 1, 2
AMX_COMM_ID_BYTES = 128

_lib = None


def lib():
    """Load librasr_amd.so; raises if it has not been built (there is no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("rasr_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc, gfx950). This package has no CPU fallback." % LIB_PATH)
        # When torch is installed its bundled HIP runtime must be the one the process loads first: a process that loads
        # /opt/rocm's libamdhip64 (through this library) and torch's copy afterwards ends up with two runtimes, and torch's
        # then reports "No HIP GPUs are available".  Tests and bench use torch for device buffers, so import it up front.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the ABI symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status):
    if status != AMX_OK:
        raise AmxError(status, lib().amx_last_error().decode("utf-8", "replace"))
