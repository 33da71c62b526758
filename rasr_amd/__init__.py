"""rasr_amd -- MI355X-native acoustic front-end and emission scorers for RASR.

Python here is plumbing only (ctypes onto librasr_amd.so, torch for device buffers / streams /
torch.distributed); all arithmetic runs in the HIP kernels behind include/amx.h.  The C++
adapters a RASR maintainer links are described in INTEGRATION.md; the classes below mirror the
same reference interfaces for tests and benchmarks:

  MfccExtractor        mfcc.flow network (Tools/FeatureExtraction/share/mfcc.flow)
  VoicednessExtractor  voicedness.flow network (autocorrelation by FFT, maximal peak value)
  GmmFeatureScorer     Mm::FeatureScorer over a Mm::MixtureSet (diagonal-maximum / diagonal-sum)
  NnBatchFeatureScorer Nn::BatchFeatureScorer (nn-batch-feature-scorer)
  ScatterMatricesEstimator  Signal::ScatterMatricesEstimator (the LDA trainer's scatter-matrix pass)
  BayesClassifier      Signal::BayesClassification (signal-bayes-classification[-score]: fast VTLN, segment classifiers)
  ViterbiAligner       Search::Aligner in Viterbi mode (Speech::AlignmentNode): search, traceback and labels on the score matrix
  BaumWelchAligner     Search::Aligner in mode baum-welch: forward-backward on the score matrix, per-frame item lists with posterior weights
  StatePosteriorScorer Mm::StatePosteriorFeatureScorer (state posteriors, the tandem feature path and the discriminative accumulators' first step)
  CombinedScorer       Mm::CombinedFeatureScorer (log-linear combination of several models' score matrices)
  QuantileEqualization Signal::QuantileEqualization in segment mode (signal-quantile-equalization); QuantileEstimator: its estimate mode
  FileArchive          Core::FileArchive + Flow cache entries (feature caches between jobs; host IO)
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (AMX_ACT_NONE, AMX_ACT_RELU, AMX_ACT_SIGMOID, AMX_ACT_TANH, AMX_ACT_ELU, AMX_GMM_BATCH_FLOAT, AMX_GMM_BAUM_WELCH, AMX_GMM_MAX, AMX_GMM_SUM, AMX_GMM_VITERBI,  # noqa: F401
                   AMX_PREC_BF16, AMX_PREC_FP32, AmxError, MfccCfg)

__all__ = ["Context", "MfccExtractor", "VoicednessExtractor", "GmmFeatureScorer", "NnBatchFeatureScorer", "FileArchive", "AmxError", "read_pms", "write_pms",
           "read_nn_matrix", "write_nn_matrix", "layer_from_parameters", "prior_from_mixture_set", "gmm_estimate",
           "ScatterMatricesEstimator", "read_matrix_f64", "write_matrix_f64", "HistogramEstimator", "HistogramNormalization",
           "BayesClassifier", "ViterbiAligner", "BaumWelchAligner", "LinearSegmenter", "gather_rows", "StatePosteriorScorer", "CombinedScorer", "QuantileEqualization", "QuantileEstimator", "read_quantiles", "write_quantiles",
           "FeedForwardTrainer", "MiniBatchTrainer", "AffineFeatureTransformEstimator", "ModelTransformEstimator", "MixtureSetAdaptor", "EbwAccumulator", "EbwEstimator", "LatticePosterior", "SegmentwiseNnTrainer", "AffineFeatureTransform", "write_transform", "read_transform", "combine_nn_statistics", "prior_from_class_counts", "mean_and_deviation",
           "AMX_GMM_VITERBI", "AMX_GMM_BAUM_WELCH"]


def _ptr(a):
    """address of a numpy array or of a (device) torch tensor"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def _is_bytes(a):
    """a best-density matrix in its byte form (torch.uint8 tensor)"""
    return a is not None and not isinstance(a, np.ndarray) and a.element_size() == 1


def version():
    """amx_version(): library version, compiler, flags and the hash of the sources it was built from"""
    return _lib.lib().amx_version().decode()


class Comm:
    """The per-epoch exchange between data-parallel ranks (amx_comm_*): RCCL all-reduce of ONE flat f64 device buffer.

    rank 0 creates the 128-byte id (Comm.unique_id()) and hands it to the others -- bench.py broadcasts it through the
    torch.distributed group that also carries its barrier; a RASR trainer would use a file or its own launcher."""

    @staticmethod
    def available():
        return bool(_lib.lib().amx_comm_available())

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * _lib.AMX_COMM_ID_BYTES)()
        _lib.check(_lib.lib().amx_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, ctx, rank, world, unique_id):
        if len(unique_id) != _lib.AMX_COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % _lib.AMX_COMM_ID_BYTES)
        self.L, self.ctx = _lib.lib(), ctx
        buf = (C.c_ubyte * _lib.AMX_COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _lib.check(self.L.amx_comm_init(ctx.h, int(rank), int(world), buf, C.byref(h)))
        self.h = h
        self.rank, self.world = int(rank), int(world)
        ctx._comms.append(self)   # a communicator belongs to its context: Context.close() closes it first (amx_comm_destroy reads the context)

    def _on_torch_stream(self):
        # the tensors handed in were produced on torch's current stream: launch there (the context's own stream is not ordered against it)
        self.ctx.use_torch_stream()

    def all_reduce_f64(self, flat):
        """in-place sum over the ranks of a contiguous float64 device tensor, on torch's current stream"""
        import torch
        if flat.dtype != torch.float64 or not flat.is_contiguous() or not flat.is_cuda:
            raise ValueError("all_reduce_f64 wants a contiguous float64 device tensor")
        self._on_torch_stream()
        _lib.check(self.L.amx_comm_all_reduce_f64_dev(self.h, flat.data_ptr(), flat.numel()))
        return flat

    def counts_to_f64(self, counts, out):
        self._on_torch_stream()
        _lib.check(self.L.amx_counts_to_f64_dev(self.ctx.h, counts.data_ptr(), out.data_ptr(), counts.numel()))

    def f64_to_counts(self, src, counts):
        self._on_torch_stream()
        _lib.check(self.L.amx_f64_to_counts_dev(self.ctx.h, src.data_ptr(), counts.data_ptr(), counts.numel()))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):   # the context is gone (finalisers run in any order at shutdown): nothing left to destroy safely
                self.L.amx_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One per process and GPU (amx_ctx)."""

    def __init__(self, device=0):
        self.L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self.L.amx_init(device, C.byref(h)))
        self.h = h
        self.device = device
        self._comms = []

    def close(self):
        if getattr(self, "h", None):
            for c in list(getattr(self, "_comms", [])):
                c.close()
            self._comms = []
            self.L.amx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    CONTRACTS = {"off": 0, "fma": 1}

    def set_contract(self, contract):
        """which build of the reference the context's f32 arithmetic follows: "off" (-DMARCH=x86-64) | "fma" (RASR's default build);
        amx_set_contract.  Read by the *_dev entry points at call time and by the front-end / GMM handles at creation."""
        _lib.check(self.L.amx_set_contract(self.h, self.CONTRACTS[contract] if isinstance(contract, str) else int(contract)))
        return self

    def contract(self):
        return {0: "off", 1: "fma"}[int(self.L.amx_get_contract(self.h))]

    def use_torch_stream(self):
        """Launch on torch's current HIP stream (so torch events / allocator ordering apply)."""
        import torch
        handle = torch.cuda.current_stream(self.device).cuda_stream
        # torch's default stream is the legacy NULL stream (handle 0); amx_set_stream(NULL) would select the context's own
        # non-blocking stream, which is NOT ordered against it -> name the legacy stream explicitly (hipStreamLegacy = 1)
        _lib.check(self.L.amx_set_stream(self.h, C.c_void_p(handle if handle else 1)))

    def synchronize(self):
        _lib.check(self.L.amx_synchronize(self.h))

    def gather_scores(self, scores_dev, ld, rows, cols, n_rows=None):
        """scores_dev[rows[i] * ld + cols[i]] for host index arrays -> host float32 array (device gather + one small copy: what a
        decoder's ContextScorer::scores(list) costs against a resident score block); n_rows: rows of the block (default: the
        tensor's first dimension) -- pairs outside [n_rows x ld] are refused"""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        out = np.empty(len(rows), np.float32)
        if n_rows is None:
            n_rows = int(scores_dev.shape[0]) if scores_dev.dim() > 1 else int(scores_dev.numel() // int(ld))
        _lib.check(self.L.amx_gather_scores(self.h, scores_dev.data_ptr(), int(n_rows), int(ld), len(rows), rows.ctypes.data,
                                            cols.ctypes.data, out.ctypes.data))
        return out

    def profile(self, enable=True):
        _lib.check(self.L.amx_profile_enable(self.h, 1 if enable else 0))

    def profile_reset(self):
        _lib.check(self.L.amx_profile_reset(self.h))

    def device_clocks(self, out_dev):
        """enqueue a sample of (s_memtime, s_memrealtime) into out_dev (2 x int64 / uint64 on the device)"""
        _lib.check(self.L.amx_device_clocks_dev(self.h, _ptr(out_dev)))

    def device_clocks_xcd(self, out_dev):
        """the same per XCD: out_dev [8 x 2] int64 / uint64 on the device, zeroed by the caller"""
        _lib.check(self.L.amx_device_clocks_xcd_dev(self.h, _ptr(out_dev)))

    def profile_get(self, kernel):
        ms, n = C.c_double(), C.c_long()
        _lib.check(self.L.amx_profile_get(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def context_window(self, plan, feats, dim, left, right, out, out_stride):
        _lib.check(self.L.amx_context_window_dev(self.h, plan.h, _ptr(feats), dim, left, right, _ptr(out), out_stride))

    # ---- feature back-end: device matrices [total_frames x ld], segmented like the plan
    def normalize(self, plan, feats, in_ld, dim, out, out_ld, variance=False, length=0, right=0):
        """signal-normalization: type mean / mean-and-variance; length = 0 is the whole segment"""
        _lib.check(self.L.amx_normalize_dev(self.h, plan.h, _ptr(feats), in_ld, dim,
                                            _lib.AMX_NORM_MEAN_AND_VARIANCE if variance else _lib.AMX_NORM_MEAN, length, right, _ptr(out), out_ld))

    def normalize_ex(self, plan, feats, in_ld, dim, out, out_ld, type, level=0, length=0, right=0):
        """signal-normalization types 2 divide-by-mean, 3 level (component `level`), 4 mean-and-variance-1D"""
        _lib.check(self.L.amx_normalize_ex_dev(self.h, plan.h, _ptr(feats), in_ld, dim, type, level, length, right, _ptr(out), out_ld))

    VECTOR_NORMALIZATIONS = {"amplitude-spectrum-energy": 0, "energy": 1, "maximum": 2, "mean-energy": 3, "mean": 4, "variance": 5}

    def vector_normalize(self, kind, feats, in_ld, n, dim, out, out_ld):
        """signal-vector-f32-<kind>-normalization on [n x dim] device views (in place on the identical view is allowed)"""
        _lib.check(self.L.amx_vector_normalize_dev(self.h, self.VECTOR_NORMALIZATIONS[kind], _ptr(feats), in_ld, n, dim, _ptr(out), out_ld))

    VECTOR_FUNCTIONS = {"log": 0, "log-plus": 1, "ln": 2, "exp": 3, "power": 4, "sqrt": 5, "cos": 6, "addition": 7, "multiplication": 8,
                        "quantize": 9, "abs": 10, "minimum": 11, "maximum": 12}

    def vector_function(self, kind, parameter, feats, in_ld, n, dim, out, out_ld):
        """generic-vector-f32-<kind> on [n, dim] device views (row strides in_ld / out_ld)"""
        _lib.check(self.L.amx_vector_function_dev(self.h, self.VECTOR_FUNCTIONS[kind], float(parameter), _ptr(feats), in_ld, n, dim, _ptr(out), out_ld))

    def regression(self, plan, feats, in_ld, dim, out, out_ld, order=1, right=2):
        """signal-delay (copy margin) + signal-regression of the given order over 2 * right + 1 frames"""
        _lib.check(self.L.amx_regression_dev(self.h, plan.h, _ptr(feats), in_ld, dim, order, right, _ptr(out), out_ld))

    def matrix_multiply(self, matrix, rows, cols, feats, in_ld, T, out, out_ld):
        """signal-matrix-multiplication-f32: out[t] = M feats[t]"""
        _lib.check(self.L.amx_matrix_multiply_dev(self.h, _ptr(matrix), rows, cols, _ptr(feats), in_ld, T, _ptr(out), out_ld))

    def stats_accumulate(self, scores, T, M, best_state, counts, score_sum):
        _lib.check(self.L.amx_stats_accumulate_dev(self.h, _ptr(scores), T, M, _ptr(best_state), _ptr(counts), _ptr(score_sum)))


class _Plan:
    def __init__(self, owner, sample_offsets, warping_factors=None):
        self.owner = owner
        self.L = owner.L
        off = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        self.n_seg = len(off) - 1
        h = C.c_void_p()
        if warping_factors is None:
            _lib.check(self.L.amx_mfcc_plan_create(owner.h, self.n_seg, off.ctypes.data, C.byref(h)))
        else:  # VTLN: one of the handle's warping factors per segment
            wf = np.ascontiguousarray(np.broadcast_to(np.asarray(warping_factors, np.float64), (self.n_seg,)))
            _lib.check(self.L.amx_mfcc_plan_create_vtln(owner.h, self.n_seg, off.ctypes.data, wf.ctypes.data, C.byref(h)))
        self.h = h
        self.total_frames = int(self.L.amx_mfcc_plan_total_frames(h))
        fo = np.zeros(self.n_seg + 1, np.int64)
        _lib.check(self.L.amx_mfcc_plan_frame_offsets(h, fo.ctypes.data))
        self.frame_offsets = fo

    def __del__(self):
        try:
            if self.h:
                self.L.amx_mfcc_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass


class GammatoneExtractor:
    """signal-gammatone -> signal-temporalintegration [-> signal-spectralintegration -> generic-vector-f32-power ->
    signal-cosine-transform].  Keyword names are the fields of amx_gammatone_cfg (= the nodes' parameters)."""

    def __init__(self, ctx, **kw):
        self.ctx, self.L = ctx, (ctx.L if ctx is not None else _lib.lib())
        cfg = _lib.GammatoneCfg()
        self.L.amx_gammatone_default_cfg(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown gammatone parameter %r" % k)
            setattr(cfg, k, _tuning(v) if k == "tuning" else v)
        self.cfg = cfg
        h = C.c_void_p()
        _lib.check(self.L.amx_gammatone_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h
        info = _lib.GammatoneInfo()
        _lib.check(self.L.amx_gammatone_describe(h, C.byref(info)))
        self.info, self.n_out, self.channels = info, info.n_out, info.channels

    def __del__(self):
        try:
            if self.h:
                self.L.amx_gammatone_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def n_frames(self, n_samples):
        return int(self.L.amx_gammatone_n_frames(self.h, n_samples))

    def tables(self):
        cf, co = np.zeros(self.channels, np.float32), np.zeros((self.channels, 4), np.float32)
        _lib.check(self.L.amx_gammatone_tables(self.h, cf.ctypes.data, co.ctypes.data))
        return cf, co

    def run(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        out = np.zeros((self.n_frames(len(pcm)), self.n_out), np.float32)
        _lib.check(self.L.amx_gammatone_run(self.h, pcm.ctypes.data, len(pcm), out.ctypes.data))
        return out

    def run_batch_dev(self, sample_offsets, pcm_dev, out_dev, filtered_dev=None):
        """torch tensors on the device; sample_offsets: host int64 [n_seg + 1]"""
        off = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        _lib.check(self.L.amx_gammatone_run_batch_dev(self.h, len(off) - 1, off.ctypes.data, pcm_dev.data_ptr(), out_dev.data_ptr(),
                                                      filtered_dev.data_ptr() if filtered_dev is not None else None))


class VoicednessExtractor:
    """voicedness.flow: signal-window (rectangular) -> signal-vector-f32-resize -> mean-energy normalisation -> signal-cross-correlation
    (x = y, FFT) -> signal-peak-detection:maximal-peak-value, one f32 per frame.  Keyword names are the fields of amx_voicedness_cfg;
    normalization takes the node's words."""
    NORMALIZATIONS = {"none": _lib.AMX_XCORR_NONE, "unbiased-estimate": _lib.AMX_XCORR_UNBIASED_ESTIMATE, "upper-bound": _lib.AMX_XCORR_UPPER_BOUND}

    def __init__(self, ctx, **kw):
        self.ctx, self.L = ctx, (ctx.L if ctx is not None else _lib.lib())
        cfg = _lib.VoicednessCfg()
        self.L.amx_voicedness_default_cfg(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown voicedness parameter %r" % k)
            if k == "normalization" and isinstance(v, str):
                v = self.NORMALIZATIONS[v]
            setattr(cfg, k, _tuning(v) if k == "tuning" else v)
        self.cfg = cfg
        h = C.c_void_p()
        _lib.check(self.L.amx_voicedness_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h
        info = _lib.VoicednessInfo()
        _lib.check(self.L.amx_voicedness_describe(h, C.byref(info)))
        self.info, self.n_lags = info, info.n_lags

    def __del__(self):
        try:
            if self.h:
                self.L.amx_voicedness_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def n_frames(self, n_samples):
        return int(self.L.amx_voicedness_n_frames(self.h, n_samples))

    def run(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        out = np.zeros(self.n_frames(len(pcm)), np.float32)
        _lib.check(self.L.amx_voicedness_run(self.h, pcm.ctypes.data, len(pcm), out.ctypes.data))
        return out

    def run_batch_dev(self, sample_offsets, pcm_dev, out_dev, out_ld=1, acf_dev=None):
        """torch tensors on the device (pcm_dev float32 or int16); sample_offsets: host int64 [n_seg + 1].  Frame t's measure goes
        to out_dev.data_ptr() + 4 * t * out_ld: pass a column view of a wider matrix and its row stride."""
        off = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        fn = self.L.amx_voicedness_run_batch_dev_s16 if pcm_dev.element_size() == 2 else self.L.amx_voicedness_run_batch_dev
        _lib.check(fn(self.h, len(off) - 1, off.ctypes.data, pcm_dev.data_ptr(), out_dev.data_ptr(), int(out_ld),
                      acf_dev.data_ptr() if acf_dev is not None else None))


    def energy_dev(self, sample_offsets, pcm_dev, sum_dev, ordered_dev):
        """test-only (amx_voicedness_energy_dev): per frame the normalisation's energy sum (float64) and whether one lane added it
        in index order (int32 1) or the wave in lane order (0)"""
        off = np.ascontiguousarray(sample_offsets, dtype=np.int64)
        _lib.check(self.L.amx_voicedness_energy_dev(self.h, len(off) - 1, off.ctypes.data, pcm_dev.data_ptr(), sum_dev.data_ptr(),
                                                    ordered_dev.data_ptr()))


class MfccExtractor:
    """The mfcc.flow chain.  Keyword names follow the Flow node parameters."""

    def __init__(self, ctx, nr_cepstrum_coefficients=16, filter_width=268.258, sample_rate=16000.0, alpha=1.0,
                 length=0.025, shift=0.01, maximum_input_size=0.025, apply_scale=True, spacing=0.0,
                 warp_differential_unit=True, normalize=False, front_end="mfcc", nr_autocorrelation_coefficients=0,
                 intensity_loudness_power=0.33, type="triangular", boundary="stretch-to-cover", warping_function="mel", tuning=None,
                 warping_factors=None, vtln_limit=0.875):
        """front_end "mfcc" (mfcc.flow), "mfplp" (mfplp.flow: pass normalize=True and nr_autocorrelation_coefficients) or "plp"
        (plp.flow: MfccExtractor.plp() fills in that file's values); type / boundary / warping_function are signal-filterbank's.
        warping_factors (VTLN): the factors of warping-function = nest(linear-2(factor, vtln_limit), mel | bark), one filter bank each;
        the first is the default of every call that names none.  ctx = None: a host-only handle (tables and geometry only)."""
        self.ctx, self.L = ctx, (ctx.L if ctx is not None else _lib.lib())
        cfg = MfccCfg(sample_rate, length, shift, alpha, maximum_input_size, int(apply_scale), filter_width, spacing,
                      int(warp_differential_unit), nr_cepstrum_coefficients, int(normalize),
                      {"mfcc": 0, "mfplp": 1, "plp": 2}[front_end], int(nr_autocorrelation_coefficients), float(intensity_loudness_power),
                      {"triangular": 0, "trapeze": 1}[type], {"stretch-to-cover": 0, "include-boundary": 1, "emphasize-boundary": 2}[boundary],
                      {"mel": 0, "bark": 1}[warping_function], _tuning(tuning))
        h = C.c_void_p()
        self.warping_factors = None
        if warping_factors is None:
            _lib.check(self.L.amx_mfcc_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        else:
            wf = np.ascontiguousarray(np.atleast_1d(np.asarray(warping_factors, np.float64)))
            vt = _lib.MfccVtln(float(vtln_limit), len(wf), wf.ctypes.data)
            _lib.check(self.L.amx_mfcc_create_vtln(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(vt), C.byref(h)))
            self.warping_factors = tuple(float(f) for f in wf)
        self.h = h
        info = _lib.MfccInfo()
        _lib.check(self.L.amx_mfcc_describe(h, C.byref(info)))
        self.info = info
        self.n_ceps, self.n_filters = info.n_ceps, info.n_filters
        self.frame_len, self.frame_shift, self.fft_len = info.frame_len, info.frame_shift, info.fft_len

    def __del__(self):
        try:
            if self.h:
                self.L.amx_mfcc_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @classmethod
    def plp(cls, ctx, nr_cepstrum_coefficients=13, nr_autocorrelation_coefficients=13, sample_rate=16000.0, spacing=0.93853,
            filter_width=3.8, **kw):
        """plp.flow: 20 ms Hamming window, no preemphasis, trapeze / include-boundary / bark filter bank, equal loudness"""
        return cls(ctx, nr_cepstrum_coefficients=nr_cepstrum_coefficients, nr_autocorrelation_coefficients=nr_autocorrelation_coefficients,
                   sample_rate=sample_rate, spacing=spacing, filter_width=filter_width, alpha=0.0, length=0.02, maximum_input_size=0.02,
                   normalize=True, front_end="plp", type="trapeze", boundary="include-boundary", warping_function="bark", **kw)

    def equal_loudness(self):
        out = np.zeros(self.info.n_transform_inputs, np.float64)
        _lib.check(self.L.amx_mfcc_equal_loudness(self.h, out.ctypes.data))
        return out

    def n_frames(self, n_samples):
        return int(self.L.amx_mfcc_n_frames(self.h, n_samples))

    def frame_start_time(self, frame):
        return float(self.L.amx_mfcc_frame_start_time(self.h, frame))

    def tables(self, warping_factor=None):
        """the kernel's tables; warping_factor: those of one of the handle's VTLN factors (amx_mfcc_tables_vtln)"""
        i = self.info
        win = np.zeros(i.frame_len, np.float32)
        fs, fe, fo = np.zeros(i.n_filters, np.int32), np.zeros(i.n_filters, np.int32), np.zeros(i.n_filters + 1, np.int32)
        if warping_factor is None:
            get = self.L.amx_mfcc_tables
        else:
            get = lambda *a: self.L.amx_mfcc_tables_vtln(a[0], float(warping_factor), *a[1:])  # noqa: E731
        _lib.check(get(self.h, None, None, None, fo.ctypes.data, None, None))
        fw = np.zeros(int(fo[-1]), np.float32)
        dct = np.zeros((i.n_transform, i.n_transform_inputs), np.float32)
        _lib.check(get(self.h, win.ctypes.data, fs.ctypes.data, fe.ctypes.data, fo.ctypes.data, fw.ctypes.data, dct.ctypes.data))
        return dict(window=win, filter_start=fs, filter_end=fe, filter_offset=fo, filter_weights=fw, dct=dct)

    def run(self, pcm, warping_factor=None):
        """host path: one segment of samples -> [n_frames, n_ceps].  An int16 array goes through the s16 entry point (the samples as
        the audio file holds them, widened inside the kernel); anything else is taken as f32 sample values.  warping_factor: one of
        the handle's VTLN factors (None: the first)"""
        if warping_factor is not None:
            return self.run_batch([pcm], warping_factors=[warping_factor])[0]
        s16 = isinstance(pcm, np.ndarray) and pcm.dtype == np.int16
        pcm = np.ascontiguousarray(pcm, dtype=np.int16 if s16 else np.float32)
        out = np.zeros((self.n_frames(len(pcm)), self.n_ceps), np.float32)
        fn = self.L.amx_mfcc_run_s16 if s16 else self.L.amx_mfcc_run
        _lib.check(fn(self.h, pcm.ctypes.data, len(pcm), out.ctypes.data))
        return out

    def run_batch(self, pcms, warping_factors=None):
        """host buffers, one output per segment; warping_factors: one of the handle's VTLN factors per segment (through a device
        plan, amx_mfcc_plan_create_vtln)"""
        s16 = all(isinstance(p, np.ndarray) and p.dtype == np.int16 for p in pcms) and len(pcms) > 0
        pcms = [np.ascontiguousarray(p, dtype=np.int16 if s16 else np.float32) for p in pcms]
        if warping_factors is not None:
            import torch
            off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
            cat = np.concatenate(pcms) if len(pcms) else np.zeros(0, np.int16 if s16 else np.float32)
            pcm_dev = torch.from_numpy(cat).to(torch.device("cuda", self.ctx.device)) if len(cat) else torch.zeros(1, dtype=torch.int16 if s16 else torch.float32,
                                                                                             device=self.ctx.device)
            ceps, fo = self.run_batch_dev(off, pcm_dev, warping_factors)
            ceps = ceps.cpu().numpy()
            return [ceps[fo[u]:fo[u + 1]].copy() for u in range(len(pcms))]
        outs = [np.zeros((self.n_frames(len(p)), self.n_ceps), np.float32) for p in pcms]
        n = len(pcms)
        ip = (C.c_void_p * n)(*[p.ctypes.data for p in pcms])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        ln = np.array([len(p) for p in pcms], np.int64)
        fn = self.L.amx_mfcc_run_batch_s16 if s16 else self.L.amx_mfcc_run_batch
        _lib.check(fn(self.h, n, C.cast(ip, C.c_void_p), ln.ctypes.data, C.cast(op, C.c_void_p)))
        return outs

    def plan(self, sample_offsets, warping_factors=None):
        return _Plan(self, sample_offsets, warping_factors)

    def run_batch_dev(self, sample_offsets, pcm_dev, warping_factors=None):
        """device path in one call: concatenated PCM tensor (float32 or int16) with segment u at sample_offsets[u]..[u + 1] ->
        ([total_frames, n_ceps] tensor, frame offsets [n_seg + 1]); warping_factors: one of the handle's VTLN factors per segment"""
        import torch
        plan = self.plan(sample_offsets, warping_factors)
        ceps = torch.empty((max(plan.total_frames, 1), self.n_ceps), dtype=torch.float32, device=pcm_dev.device)
        torch.cuda.synchronize(pcm_dev.device)   # the samples may still be in flight on torch's stream
        self.run_plan(plan, pcm_dev, ceps)
        torch.cuda.synchronize(pcm_dev.device)
        return ceps[:plan.total_frames], plan.frame_offsets

    def run_plan(self, plan, pcm_dev, ceps_dev):
        """device path: concatenated PCM tensor (float32 or int16) -> [total_frames, n_ceps] tensor (both resident in HBM)"""
        import torch
        if pcm_dev.dtype == torch.int16:
            _lib.check(self.L.amx_mfcc_run_plan_dev_s16(self.h, plan.h, _ptr(pcm_dev), _ptr(ceps_dev)))
        else:
            _lib.check(self.L.amx_mfcc_run_plan_dev(self.h, plan.h, _ptr(pcm_dev), _ptr(ceps_dev)))


def _tuning(t):
    """tuning=None | "key=value,..." | dict -> bytes for the `tuning` field of the ABI structs (A/B runs and tests)"""
    if not t:
        return None
    if isinstance(t, dict):
        t = ",".join("%s=%s" % (k, v) for k, v in t.items())
    return t.encode()


def _gmm_struct(model, mixture_weight_scale, gaussian_scale, keep, tuning=None):
    m = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in model.items()}
    assert m["mix_offsets"].dtype == np.uint32 and m["dens_index"].dtype == np.uint32
    assert m["dens_mean"].dtype == np.uint32 and m["dens_cov"].dtype == np.uint32
    assert m["log_weight"].dtype == np.float64 and m["means"].dtype == np.float32 and m["variances"].dtype == np.float32
    keep.append(m)
    return _lib.GmmModel(int(m["dim"]), len(m["mix_offsets"]) - 1, len(m["dens_mean"]), m["means"].shape[0],
                         m["variances"].shape[0], m["mix_offsets"].ctypes.data, m["dens_index"].ctypes.data,
                         m["log_weight"].ctypes.data, m["dens_mean"].ctypes.data, m["dens_cov"].ctypes.data,
                         m["means"].ctypes.data, m["variances"].ctypes.data, mixture_weight_scale, gaussian_scale, _tuning(tuning))


class GmmFeatureScorer:
    """Mm::FeatureScorer over a mixture set; feature_scorer_type in {"diagonal-maximum", "diagonal-sum",
    "batch-diagonal-maximum-float", "SIMD-diagonal-maximum"}.

    model: dict(dim, mix_offsets u32[M+1], dens_index u32[sumK], log_weight f64[sumK], dens_mean u32[D],
    dens_cov u32[D], means f32[n_mean,dim], variances f32[n_cov,dim]).
    """

    def __init__(self, ctx, model, feature_scorer_type="diagonal-maximum", mixture_weight_scale=1.0, gaussian_scale=1.0, tuning=None):
        # ctx = None: host-only handle (prepared tables, accumulator files); scoring then fails with AMX_ERR_STATE
        self.ctx, self.L = ctx, (ctx.L if ctx is not None else _lib.lib())
        self.mode = {"diagonal-maximum": AMX_GMM_MAX, "diagonal-sum": AMX_GMM_SUM,
                     "batch-diagonal-maximum-float": AMX_GMM_BATCH_FLOAT, "SIMD-diagonal-maximum": _lib.AMX_GMM_SIMD, "batch-diagonal-maximum-int": _lib.AMX_GMM_BATCH_INT,
                     "batch-diagonal-maximum-fast": _lib.AMX_GMM_BATCH_INT, "preselection-batch-float": _lib.AMX_GMM_PRESELECTION_FLOAT,
                     "preselection-batch-int": _lib.AMX_GMM_PRESELECTION_INT}[feature_scorer_type]
        keep = []
        st = _gmm_struct(model, mixture_weight_scale, gaussian_scale, keep, tuning)   # tuning: amx_gmm_model.tuning, e.g. "screen=0"
        h = C.c_void_p()
        _lib.check(self.L.amx_gmm_create(ctx.h if ctx is not None else None, C.byref(st), C.byref(h)))
        self.h = h
        self.n_mix, self.dim = st.n_mix, st.dim
        self._nk, self._ncov = int(keep[0]["mix_offsets"][-1]), st.n_cov

    def __del__(self):
        try:
            if self.h:
                self.L.amx_gmm_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def nMixtures(self):
        return int(self.L.amx_gmm_n_mixtures(self.h))

    def dimension(self):
        return int(self.L.amx_gmm_dimension(self.h))

    def tables(self):
        a, b, c = np.zeros(self._nk, np.float32), np.zeros((self._ncov, self.dim), np.float32), np.zeros(self._ncov, np.float32)
        _lib.check(self.L.amx_gmm_tables(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data))
        return a, b, c

    def score(self, feats, want_best=True):
        """host path: feats [T, dim] -> (scores [T, M], best_density [T, M])"""
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        T = feats.shape[0]
        sc = np.zeros((T, self.n_mix), np.float32)
        best = np.zeros((T, self.n_mix), np.uint32) if want_best else None
        _lib.check(self.L.amx_gmm_score(self.h, self.mode, feats.ctypes.data, T, sc.ctypes.data, _ptr(best)))
        return (sc, best) if want_best else sc

    def score_dev(self, feats_dev, T, scores_dev, best_dev=None):
        _lib.check(self.L.amx_gmm_score_dev(self.h, self.mode, _ptr(feats_dev), T, _ptr(scores_dev), _ptr(best_dev)))

    def score_stats_dev(self, feats_dev, T, scores_dev, best_density, best_state, counts, score_sum):
        """diagonal-maximum scores plus best state / per-state counts / sum of best scores (arg-min fused where possible); a
        one-byte best_density tensor (torch.uint8) selects the byte form of the matrix (amx_gmm_score_stats_u8_dev)"""
        fn = self.L.amx_gmm_score_stats_u8_dev if _is_bytes(best_density) else self.L.amx_gmm_score_stats_dev
        _lib.check(fn(self.h, _ptr(feats_dev), T, _ptr(scores_dev), _ptr(best_density), _ptr(best_state), _ptr(counts), _ptr(score_sum)))

    def simd_scaling(self):
        """quantisation scaling factor of the SIMD-diagonal-maximum scorer"""
        return float(self.L.amx_gmm_simd_scaling(self.h))

    def set_preselection(self, clusters=256, select_clusters=32, iterations=5, backoff_score=40000.0):
        """density-clustering parameters of preselection-batch-float (Mm/DensityClustering.cc:21-35)"""
        _lib.check(self.L.amx_gmm_set_preselection(self.h, clusters, select_clusters, iterations, backoff_score))

    def preselection_clustering(self):
        """(cluster index of every mixture entry uint32[sum K], cluster means float32[n_clusters, dim])"""
        fn = self.L.amx_gmm_preselection_int_clustering if self.mode == _lib.AMX_GMM_PRESELECTION_INT else self.L.amx_gmm_preselection_clustering
        n = C.c_int(0)
        _lib.check(fn(self.h, C.byref(n), None, None))
        cof = np.zeros(self._nk, np.uint32)
        cm = np.zeros((n.value, self.dim), np.float32)
        _lib.check(fn(self.h, C.byref(n), cof.ctypes.data, cm.ctypes.data))
        return cof, cm

    def screen_counts(self, enable=True):
        """(densities evaluated exactly, (frame, mixture) pairs) of the fused screened scorer since the last call; sets counting on / off"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        _lib.check(self.L.amx_gmm_screen_counts(self.h, 1 if enable else 0, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def accumulator_size(self):
        return int(self.L.amx_gmm_accumulator_size(self.h))

    def write_accumulator(self, acc, path):
        """flat f64 accumulator (numpy, host) -> binary MIXSET estimator file (Mm::MixtureSetEstimator::write)"""
        a = np.ascontiguousarray(acc, dtype=np.float64)
        if a.size != self.accumulator_size():
            raise ValueError("accumulator has %d entries, expected %d" % (a.size, self.accumulator_size()))
        _lib.check(self.L.amx_gmm_accumulator_write(self.h, a.ctypes.data, os.fsencode(path)))

    def read_accumulator(self, path):
        a = np.zeros(self.accumulator_size(), np.float64)
        _lib.check(self.L.amx_gmm_accumulator_read(self.h, os.fsencode(path), a.ctypes.data))
        return a

    def best_density_dev(self, feats_dev, T, mixture_dev, best_density_dev, scores_dev=None):
        """AssigningContextScorer::bestDensity(e) for one mixture per frame: best_density_dev[t] (u32) and, optionally, scores_dev[t]"""
        _lib.check(self.L.amx_gmm_best_density_dev(self.h, _ptr(feats_dev), T, _ptr(mixture_dev), _ptr(best_density_dev), _ptr(scores_dev)))

    def accumulate_dev(self, feats_dev, T, mixture_dev, best_density_dev, best_density_ld, acc_dev):
        """Viterbi statistics (weights, sum x, sum x^2 in f64) into the flat accumulator acc_dev; best_density_dev u32 or bytes"""
        fn = self.L.amx_gmm_accumulate_u8_dev if _is_bytes(best_density_dev) else self.L.amx_gmm_accumulate_dev
        _lib.check(fn(self.h, _ptr(feats_dev), T, _ptr(mixture_dev), _ptr(best_density_dev), best_density_ld, _ptr(acc_dev)))


    def accumulate_weighted_dev(self, mode, feats_dev, T, mixture_dev, weight_dev, best_density_dev, best_density_ld, acc_dev):
        """weighted Viterbi (mode AMX_GMM_VITERBI) or Baum-Welch (AMX_GMM_BAUM_WELCH) statistics; weight_dev f64 per frame or None"""
        _lib.check(self.L.amx_gmm_accumulate_weighted_dev(self.h, mode, _ptr(feats_dev), T, _ptr(mixture_dev), _ptr(weight_dev),
                                                          _ptr(best_density_dev), best_density_ld, _ptr(acc_dev)))


class NnBatchFeatureScorer:
    """Nn::BatchFeatureScorer: Ws[l] is [out, in] (RASR weights_[0] is the same memory, [in x out] col-major)."""

    def __init__(self, ctx, Ws, biases, activations, log_prior=None, priori_scale=1.0, precision="bf16", class_to_output=None, tuning=None,
                 preprocessing=None, maxout=None):
        """class_to_output: Nn::ClassLabelWrapper mapping [n_classes] (emission -> network output, -1 = disregarded class)
        preprocessing: layers in front of layer 0, in order: "logarithm", or ("mean-and-variance-normalization", mean, stddev)
        maxout: {layer: G (maxout-size: out_dim / G units per group) or [group sizes] (maxout-sizes)} -- a maxoutvar behind that layer;
        activations may hold AMX_ACT_ELU (4).  Either argument goes through amx_ffnn_create_ex (include/amx.h)."""
        self.ctx, self.L = ctx, ctx.L
        n = len(Ws)
        self._Ws = [np.ascontiguousarray(w, dtype=np.float32) for w in Ws]
        self._bs = [np.ascontiguousarray(b, dtype=np.float32) for b in biases]
        self._ind = np.array([w.shape[1] for w in self._Ws], np.int32)
        self._outd = np.array([w.shape[0] for w in self._Ws], np.int32)
        self._act = np.array(activations, np.int32)
        self._lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float32)
        self._map = None if class_to_output is None else np.ascontiguousarray(class_to_output, dtype=np.int32)
        Wp = (C.c_void_p * n)(*[w.ctypes.data for w in self._Ws])
        Bp = (C.c_void_p * n)(*[b.ctypes.data for b in self._bs])
        st = _lib.FfnnModel(n, self._ind.ctypes.data, self._outd.ctypes.data, C.cast(Wp, C.c_void_p), C.cast(Bp, C.c_void_p),
                            self._act.ctypes.data, _ptr(self._lp), priori_scale,
                            {"fp32": AMX_PREC_FP32, "bf16": AMX_PREC_BF16, "bf16x3": _lib.AMX_PREC_BF16X3, "f16mx": _lib.AMX_PREC_F16MX}[precision],
                            0 if self._map is None else len(self._map), _ptr(self._map), _tuning(tuning))   # e.g. tuning="tile=3"
        h = C.c_void_p()
        if preprocessing or maxout:
            ext = self._layers(n, preprocessing or [], maxout or {})
            _lib.check(self.L.amx_ffnn_create_ex(ctx.h, C.byref(st), C.byref(ext), C.byref(h)))
        else:
            _lib.check(self.L.amx_ffnn_create(ctx.h, C.byref(st), C.byref(h)))
        self.h = h
        self.in_dim, self.out_dim = int(self._ind[0]), int(self.L.amx_ffnn_output_dim(h))
        self.hidden_dim = int(self.L.amx_ffnn_hidden_dim(h))

    def _layers(self, n, preprocessing, maxout):
        """amx_ffnn_layers for the preprocessing list and the maxout map (the arrays stay referenced by self)"""
        names = {"logarithm": _lib.AMX_NN_PRE_LOGARITHM, "mean-and-variance-normalization": _lib.AMX_NN_PRE_MEAN_AND_VARIANCE}
        types, vecs = [], []
        for p in preprocessing:
            p = (p,) if isinstance(p, str) else tuple(p)
            if p[0] not in names:
                raise ValueError("unknown preprocessing layer %r (expected %s)" % (p[0], " | ".join(names)))
            types.append(names[p[0]])
            vecs.append([None if v is None else np.ascontiguousarray(v, dtype=np.float32) for v in p[1:3]] if len(p) >= 3 else [None, None])
        self._pre_vecs = vecs
        self._pre_type = np.array(types, np.int32)
        self._pre_mean = (C.c_void_p * max(len(vecs), 1))(*[_ptr(v[0]) for v in vecs])
        self._pre_std = (C.c_void_p * max(len(vecs), 1))(*[_ptr(v[1]) for v in vecs])
        items = maxout.items() if isinstance(maxout, dict) else enumerate(maxout)
        groups, sizes = np.zeros(n, np.int32), [None] * n
        for l, g in items:
            if g is None or (np.isscalar(g) and int(g) == 0):
                continue
            if np.isscalar(g):
                groups[l] = int(g)
            else:
                sizes[l] = np.ascontiguousarray(g, dtype=np.int32)
                groups[l] = len(sizes[l])
        self._mo_groups, self._mo_sizes_arr = groups, sizes
        self._mo_sizes = (C.c_void_p * n)(*[_ptr(v) for v in sizes])
        return _lib.FfnnLayers(len(types), _ptr(self._pre_type) if types else None, C.cast(self._pre_mean, C.c_void_p),
                               C.cast(self._pre_std, C.c_void_p), self._mo_groups.ctypes.data, C.cast(self._mo_sizes, C.c_void_p))

    def __del__(self):
        try:
            if self.h:
                self.L.amx_ffnn_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def nMixtures(self):
        return int(self.L.amx_ffnn_output_dim(self.h))

    def score(self, feats):
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        T = feats.shape[0]
        out = np.zeros((T, self.out_dim), np.float32)
        _lib.check(self.L.amx_ffnn_score(self.h, feats.ctypes.data, T, out.ctypes.data))
        return out

    def forward_hidden_dev(self, feats_dev, feats_stride, T, act_dev):
        """Nn::OnDemandFeatureScorer::forwardHiddenLayers for T frames: act_dev [T, hidden_dim] f32"""
        _lib.check(self.L.amx_ffnn_forward_hidden_dev(self.h, _ptr(feats_dev), feats_stride, T, _ptr(act_dev)))

    def forward_dev(self, feats_dev, feats_stride, T, out_dev, top="softmax"):
        """Nn::NeuralNetworkForwardNode: the top layer's output [T, out_last]; top "linear" (W x + b - alpha log prior) or "softmax"""
        _lib.check(self.L.amx_ffnn_forward_dev(self.h, _ptr(feats_dev), feats_stride, T, _ptr(out_dev), {"linear": 0, "softmax": 1}[top]))

    def score_on_demand_dev(self, act_dev, n_pairs, frame_dev, emission_dev, scores_dev):
        """output layer for (frame, emission) pairs only: scores_dev [n_pairs]"""
        _lib.check(self.L.amx_ffnn_score_on_demand_dev(self.h, _ptr(act_dev), n_pairs, _ptr(frame_dev), _ptr(emission_dev), _ptr(scores_dev)))

    def effective_precision(self):
        """(precision the handle computes in, block-maximum statistic of its weights): "f16mx" requested on heavy-tailed weights runs "bf16x3"""
        r = C.c_double(0.0)
        p = self.L.amx_ffnn_precision(self.h, C.byref(r))
        return {0: "fp32", 1: "bf16", 2: "bf16x3", 3: "f16mx"}[p], float(r.value)

    def wait_dev(self):
        """amx_ffnn_wait_dev: waits for the handle's stream; raises if a pass of an f16mx scorer left the f16 range"""
        _lib.check(self.L.amx_ffnn_wait_dev(self.h))

    def score_dev(self, feats_dev, feats_stride, T, scores_dev):
        _lib.check(self.L.amx_ffnn_score_dev(self.h, _ptr(feats_dev), feats_stride, T, _ptr(scores_dev)))

    def score_stats_dev(self, feats_dev, feats_stride, T, scores_dev, best_state, counts, score_sum):
        """scores plus best state / per-state counts / sum of best scores (arg-min fused into the output layer)"""
        _lib.check(self.L.amx_ffnn_score_stats_dev(self.h, _ptr(feats_dev), feats_stride, T, _ptr(scores_dev), _ptr(best_state),
                                                   _ptr(counts), _ptr(score_sum)))


def dc_detection(pcm, sample_rate=16000.0, min_dc_length=0.0125, max_dc_increment=0.9, min_non_dc_segment_length=0.02, maximal_output_size=4096,
                 merge=False):
    """signal-dc-detection over one segment (host): [(first sample, length)] of the blocks the node lets through; merge=True joins blocks
    without a gap (the ranges to frame separately)"""
    x = np.ascontiguousarray(pcm, dtype=np.float32)
    L = _lib.lib()
    n = C.c_longlong(0)
    args = (x.ctypes.data if len(x) else None, len(x), float(sample_rate), float(min_dc_length), float(max_dc_increment),
            float(min_non_dc_segment_length), int(maximal_output_size), int(merge))
    _lib.check(L.amx_dc_detection(*args, None, None, 0, C.byref(n)))
    st, ln = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
    _lib.check(L.amx_dc_detection(*args, st.ctypes.data, ln.ctypes.data, n.value, C.byref(n)))
    return list(zip(st.tolist(), ln.tolist()))


def class_labels_init(n_classes, disregard=()):
    """Nn::ClassLabelWrapper::initMapping: (mapping int32[n_classes], number of classes to accumulate)"""
    dis = np.ascontiguousarray(list(disregard), dtype=np.int32)
    mapping = np.zeros(n_classes, np.int32)
    nt = C.c_int(0)
    _lib.check(_lib.lib().amx_class_labels_init(n_classes, _ptr(dis) if len(dis) else None, len(dis), mapping.ctypes.data, C.byref(nt)))
    return mapping, int(nt.value)


def _read_vector(fn, path, ctype, dtype):
    n, p = C.c_int(0), C.c_void_p()
    L = _lib.lib()
    _lib.check(getattr(L, fn)(os.fsencode(path), C.byref(n), C.byref(p)))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(n.value, 1),))[:n.value].astype(dtype).copy()
    finally:
        L.amx_free(p)


def read_prior(path):
    """Nn::Prior::read: Math::Vector<f32> file (xml, or bin:<path>) -> log-prior float32[n]"""
    return _read_vector("amx_nn_vector_read_f32", path, C.c_float, np.float32)


def write_prior(path, log_prior):
    v = np.ascontiguousarray(log_prior, dtype=np.float32)
    _lib.check(_lib.lib().amx_nn_vector_write_f32(os.fsencode(path), len(v), v.ctypes.data))


def read_class_labels(path):
    """Nn::ClassLabelWrapper::load: Math::Vector<s32> xml file -> mapping int32[n_classes]"""
    return _read_vector("amx_nn_vector_read_s32", path, C.c_int, np.int32)


def read_maxout_sizes(path):
    """maxoutvar's `maxout-sizes`: Math::Vector<u32> file (xml, or bin:<path>) -> group sizes uint32[G]"""
    return _read_vector("amx_nn_vector_read_u32", path, C.c_uint32, np.uint32)


def write_class_labels(path, mapping):
    v = np.ascontiguousarray(mapping, dtype=np.int32)
    _lib.check(_lib.lib().amx_nn_vector_write_s32(os.fsencode(path), len(v), v.ctypes.data))


def precomputed_score_dev(ctx, feats_dev, feats_stride, T, n_classes, class_to_output_dev, log_prior_dev, prior_scale, scores_dev):
    """Nn::PrecomputedFeatureScorer: -x[out(e)] + alpha * logPrior[out(e)]"""
    _lib.check(ctx.L.amx_precomputed_score_dev(ctx.h, _ptr(feats_dev), feats_stride, T, n_classes, _ptr(class_to_output_dev),
                                               _ptr(log_prior_dev), prior_scale, _ptr(scores_dev)))


def _mixture_set_to_dict(h):
    L = _lib.lib()
    try:
        v = _lib.GmmModel()
        _lib.check(L.amx_mixture_set_view(h, C.byref(v)))
        nk_arr = np.ctypeslib.as_array(C.cast(v.mix_offsets, C.POINTER(C.c_uint32)), shape=(v.n_mix + 1,)).copy()
        nk = int(nk_arr[-1])

        def arr(p, t, shape):
            n = int(np.prod(shape))
            if n == 0:
                return np.zeros(shape, np.dtype(t))
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=shape).copy()

        return dict(dim=v.dim, mix_offsets=nk_arr, dens_index=arr(v.dens_index, C.c_uint32, (nk,)),
                    log_weight=arr(v.log_weight, C.c_double, (nk,)), dens_mean=arr(v.dens_mean, C.c_uint32, (v.n_dens,)),
                    dens_cov=arr(v.dens_cov, C.c_uint32, (v.n_dens,)), means=arr(v.means, C.c_float, (v.n_mean, v.dim)),
                    variances=arr(v.variances, C.c_float, (v.n_cov, v.dim)))
    finally:
        L.amx_mixture_set_destroy(h)


def read_pms(path):
    """text mixture set -> model dict (see GmmFeatureScorer)"""
    h = C.c_void_p()
    _lib.check(_lib.lib().amx_pms_read(path.encode(), C.byref(h)))
    return _mixture_set_to_dict(h)


def gmm_estimate(model, acc, **cfg):
    """Re-estimation (and, with split=True, splitting) from the flat f64 statistics: Mm::AbstractMixtureSetEstimator::estimate /
    Mm::MixtureSetSplitter::split.  `model` is the model dict the statistics were accumulated with; keyword arguments are the
    fields of amx_gmm_estimate_cfg.  Returns the new model dict."""
    L = _lib.lib()
    c = _lib.GmmEstimateCfg()
    L.amx_gmm_estimate_cfg_default(C.byref(c))
    for k, v in cfg.items():
        if not hasattr(c, k):
            raise TypeError("unknown estimate option %r" % k)
        setattr(c, k, v)
    keep = []
    st = _gmm_struct(model, 1.0, 1.0, keep)
    a = np.ascontiguousarray(acc, dtype=np.float64)
    nk = int(np.asarray(model["mix_offsets"])[-1])
    need = nk + st.n_mean * (1 + st.dim) + st.n_cov * (1 + st.dim)
    if a.size != need:
        raise ValueError("accumulator has %d entries, expected %d" % (a.size, need))
    h = C.c_void_p()
    _lib.check(L.amx_gmm_estimate(C.byref(st), a.ctypes.data, C.byref(c), C.byref(h)))
    return _mixture_set_to_dict(h)


def write_pms(model, path):
    keep = []
    st = _gmm_struct(model, 1.0, 1.0, keep)
    _lib.check(_lib.lib().amx_pms_write(C.byref(st), path.encode()))



class FileArchive:
    """Core::FileArchive ("SP_ARC1") over the C ABI: a RASR feature cache file.  ``mode`` "r" or "w" (read-write,
    created when missing).  Mirrors the calls of Flow::Cache / Core::Archive (src/Flow/Cache.cc, src/Core/Archive.hh)."""

    def __init__(self, path, mode="r"):
        self._h = C.c_void_p()
        m = {"r": _lib.AMX_ARCHIVE_READ, "w": _lib.AMX_ARCHIVE_WRITE}[mode]
        _lib.check(_lib.lib().amx_archive_open(os.fsencode(path), m, C.byref(self._h)))

    def close(self):
        if self._h:
            h, self._h = self._h, C.c_void_p()
            _lib.check(_lib.lib().amx_archive_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def files(self):
        """[(name, size, compressed_size)] in archive order"""
        L, out = _lib.lib(), []
        for i in range(L.amx_archive_n_files(self._h)):
            name, size, comp = C.c_char_p(), C.c_uint32(), C.c_uint32()
            _lib.check(L.amx_archive_file_info(self._h, i, C.byref(name), C.byref(size), C.byref(comp)))
            out.append((name.value.decode(), size.value, comp.value))
        return out

    def __contains__(self, name):
        return bool(_lib.lib().amx_archive_has_file(self._h, name.encode()))

    def read_file(self, name):
        L, p, n = _lib.lib(), C.c_void_p(), C.c_size_t()
        _lib.check(L.amx_archive_read_file(self._h, name.encode(), C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            L.amx_free(p)

    def write_file(self, name, data, compress=False):
        data = bytes(data)
        _lib.check(_lib.lib().amx_archive_write_file(self._h, name.encode(), data, len(data), int(compress)))

    def remove_file(self, name):
        _lib.check(_lib.lib().amx_archive_remove_file(self._h, name.encode()))

    # ---- Flow cache entries (vector-f32 packets)
    def write_features(self, segment, feats, times, gather=0xFFFFFFFF, compress=False, attributes=None):
        """feats [n, dim] f32, times [n, 2] f64 (start, end); attributes: optional {name: value} -> '<segment>.attribs'"""
        x = np.ascontiguousarray(feats, dtype=np.float32)
        t = np.ascontiguousarray(times, dtype=np.float64)
        if x.ndim != 2 or t.shape != (x.shape[0], 2):
            raise ValueError("write_features: feats [n, dim] and times [n, 2] expected")
        L = _lib.lib()
        if attributes is not None:
            names = (C.c_char_p * len(attributes))(*[k.encode() for k in attributes])
            vals = (C.c_char_p * len(attributes))(*[str(v).encode() for v in attributes.values()])
            _lib.check(L.amx_feature_cache_write_attributes(self._h, segment.encode(), len(attributes), names, vals, int(compress)))
        _lib.check(L.amx_feature_cache_write(self._h, segment.encode(), x.shape[0], x.shape[1], x.ctypes.data, t.ctypes.data,
                                             int(gather), int(compress)))

    def read_features(self, segment):
        """-> (feats [n, dim] f32, times [n, 2] f64)"""
        L = _lib.lib()
        n, d, px, pt = C.c_int(), C.c_int(), C.c_void_p(), C.c_void_p()
        _lib.check(L.amx_feature_cache_read(self._h, segment.encode(), C.byref(n), C.byref(d), C.byref(px), C.byref(pt)))
        try:
            cnt = n.value * d.value
            x = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_float)), shape=(max(cnt, 1),))[:cnt].copy()
            t = np.ctypeslib.as_array(C.cast(pt, C.POINTER(C.c_double)), shape=(max(2 * n.value, 1),))[:2 * n.value].copy()
            return x.reshape(n.value, d.value), t.reshape(n.value, 2)
        finally:
            L.amx_free(px)
            L.amx_free(pt)

    def read_attributes(self, segment):
        """'<segment>.attribs' -> {name: value}"""
        import xml.etree.ElementTree as ET
        L, p = _lib.lib(), C.c_void_p()
        _lib.check(L.amx_feature_cache_read_attributes(self._h, segment.encode(), C.byref(p)))
        try:
            root = ET.fromstring(C.string_at(p).decode())
        finally:
            L.amx_free(p)
        return {e.get("name"): e.get("value") for e in root.iter("flow-attribute")}


def read_nn_matrix(path):
    """binary Math::Matrix<f32> (RASR NN layer parameter file) -> numpy [rows, cols]"""
    L = _lib.lib()
    r, c, p = C.c_int(), C.c_int(), C.c_void_p()
    _lib.check(L.amx_nn_matrix_read(path.encode(), C.byref(r), C.byref(c), C.byref(p)))
    try:
        n = r.value * c.value
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(max(n, 1),))[:n].copy()
        return a.reshape(r.value, c.value)
    finally:
        L.amx_free(p)


def write_nn_matrix(path, m):
    m = np.ascontiguousarray(m, dtype=np.float32)
    _lib.check(_lib.lib().amx_nn_matrix_write(path.encode(), m.shape[0], m.shape[1], m.ctypes.data))


def read_matrix_f64(path):
    """binary Math::Matrix<f64> (a scatter matrix as RASR's LDA tool reads it, optional "bin:" prefix) -> numpy [rows, cols]"""
    L = _lib.lib()
    r, c, p = C.c_int(), C.c_int(), C.c_void_p()
    _lib.check(L.amx_matrix_read_f64(os.fsencode(path), C.byref(r), C.byref(c), C.byref(p)))
    try:
        n = r.value * c.value
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(max(n, 1),))[:n].copy()
        return a.reshape(r.value, c.value)
    finally:
        L.amx_free(p)


def write_matrix_f64(path, m):
    m = np.ascontiguousarray(m, dtype=np.float64)
    _lib.check(_lib.lib().amx_matrix_write_f64(os.fsencode(path), m.shape[0], m.shape[1], m.ctypes.data))


class ScatterMatricesEstimator:
    """Signal::ScatterMatricesEstimator: the flat f64 accumulator [dim (dim + 1) / 2 square sums (lower triangle) | n_classes x dim class
    sums | n_classes counts], its corpus pass on the device, its file and its finalize step.  ctx may be None for host-only use
    (files, finalize)."""

    def __init__(self, ctx, dim, n_classes):
        self.L = _lib.lib()
        self.ctx, self.dim, self.n_classes = ctx, int(dim), int(n_classes)
        if self.accumulator_size() == 0:
            raise ValueError("ScatterMatricesEstimator: dim %d must lie in [1, 1024] and n_classes %d be positive" % (self.dim, self.n_classes))

    def accumulator_size(self):
        return int(self.L.amx_scatter_accumulator_size(self.dim, self.n_classes))

    def accumulate_dev(self, feats_dev, in_ld, T, class_dev, acc_dev, weight_dev=None):
        """add T frames feats_dev[t * in_ld + 0 .. dim) (f32) of class class_dev[t] (u32; >= n_classes: skipped) and weight
        weight_dev[t] (f32, None: 1) into the flat accumulator acc_dev (f64, accumulator_size() entries)"""
        if self.ctx is None:
            raise RuntimeError("ScatterMatricesEstimator.accumulate_dev: created without a context")
        _lib.check(self.L.amx_scatter_accumulate_dev(self.ctx.h, _ptr(feats_dev), int(in_ld), int(T), self.dim, _ptr(class_dev), self.n_classes,
                                                     _ptr(weight_dev), _ptr(acc_dev)))

    def _host(self, acc_host):
        a = np.ascontiguousarray(acc_host, dtype=np.float64)
        if a.size != self.accumulator_size():
            raise ValueError("accumulator has %d entries, expected %d" % (a.size, self.accumulator_size()))
        return a

    def finalize(self, acc_host, normalize=False):
        """(between-class, within-class, total) scatter matrices, each f64 [dim, dim]; normalize = `shall-normalize`"""
        a = self._host(acc_host)
        out = [np.zeros((self.dim, self.dim), np.float64) for _ in range(3)]
        _lib.check(self.L.amx_scatter_finalize(self.dim, self.n_classes, a.ctypes.data, 1 if normalize else 0, *[m.ctypes.data for m in out]))
        return tuple(out)

    def write(self, acc_host, path):
        """flat accumulator (numpy, host) -> the accumulator file of ScatterMatricesEstimator::write (`new-accumulator-file`)"""
        a = self._host(acc_host)
        _lib.check(self.L.amx_scatter_accumulator_write(self.dim, self.n_classes, a.ctypes.data, os.fsencode(path)))

    @staticmethod
    def read(path):
        """accumulator file -> (dim, n_classes, flat accumulator)"""
        L = _lib.lib()
        d, n, p = C.c_int(), C.c_int(), C.c_void_p()
        _lib.check(L.amx_scatter_accumulator_read(os.fsencode(path), C.byref(d), C.byref(n), C.byref(p)))
        try:
            size = int(L.amx_scatter_accumulator_size(d.value, n.value))
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(size,)).copy()
        finally:
            L.amx_free(p)
        return d.value, n.value, a


def _lookup_table(fn, *head):
    """(bucket_size, offset, values f32) of one table through an amx_*_table style getter (size first, then the values)"""
    bs, off, n = C.c_float(), C.c_int(), C.c_int()
    _lib.check(fn(*head, C.byref(bs), C.byref(off), C.byref(n), None))
    v = np.zeros(n.value, np.float32)
    _lib.check(fn(*head, C.byref(bs), C.byref(off), C.byref(n), v.ctypes.data))
    return np.float32(bs.value), off.value, v


class HistogramEstimator:
    """Speech::HistogramEstimator for ONE corpus key: a Signal::HistogramVector<f32> of `dim` histograms (amx_histogram).  ctx may be
    None for host-only use (files, tables, accumulate on the host)."""

    def __init__(self, ctx, dim, bucket_size=0.0002, _handle=None):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        if _handle is None:
            _handle = C.c_void_p()
            _lib.check(self.L.amx_histogram_create(ctx.h if ctx is not None else None, int(dim), float(bucket_size), C.byref(_handle)))
        self.h = _handle
        self.dim = self.describe()["dim"]

    def close(self):
        if self.h:
            self.L.amx_histogram_destroy(self.h)
            self.h = None

    __del__ = close

    def describe(self):
        info = _lib.HistogramInfo()
        _lib.check(self.L.amx_histogram_describe(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def attach(self, ctx):
        _lib.check(self.L.amx_histogram_attach(self.h, ctx.h))
        self.ctx = ctx

    def accumulate_dev(self, feats_dev, in_ld, T):
        """add T frames feats_dev[t * in_ld + 0 .. dim) (f32, device) of this key"""
        _lib.check(self.L.amx_histogram_accumulate_dev(self.h, _ptr(feats_dev), int(in_ld), int(T)))

    def accumulate(self, feats):
        """the same for a host array [T, dim], in plain C++"""
        x = np.ascontiguousarray(feats, dtype=np.float32)
        _lib.check(self.L.amx_histogram_accumulate(self.h, x.ctypes.data, x.shape[1] if x.ndim == 2 else self.dim, x.size // max(1, x.shape[-1])))

    def table(self, d):
        """(bucket_size, offset, values) of dimension d"""
        return _lookup_table(self.L.amx_histogram_table, self.h, int(d))

    def cdf(self, d):
        return _lookup_table(self.L.amx_histogram_cdf, self.h, int(d))

    def percentile(self, d, percent):
        v = C.c_float()
        _lib.check(self.L.amx_histogram_percentile(self.h, int(d), float(percent), C.byref(v)))
        return np.float32(v.value)

    def write(self, path):
        """the per-key file of the histograms cache == a training-histogram file (HistogramVector::write)"""
        _lib.check(self.L.amx_histogram_write(self.h, os.fsencode(path)))

    @classmethod
    def read(cls, path, ctx=None):
        h = C.c_void_p()
        _lib.check(_lib.lib().amx_histogram_read(os.fsencode(path), C.byref(h)))
        e = cls(None, 0, _handle=h)
        if ctx is not None:
            e.attach(ctx)
        return e


class HistogramNormalization:
    """Signal::HistogramNormalization (the `signal-histogram-normalization` node's arithmetic): inverse CDFs from one training histogram, or
    from several interpolated with set_scales; test CDFs per corpus key (add_key); apply_dev normalises all segments in one launch."""

    def __init__(self, ctx, training, probability_bucket_size=0.0):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        training = list(training)
        arr = (C.c_void_p * len(training))(*[t.h for t in training])
        h = C.c_void_p()
        _lib.check(self.L.amx_histnorm_create(ctx.h if ctx is not None else None, len(training), arr, float(probability_bucket_size), C.byref(h)))
        self.h = h
        self.dim = training[0].dim

    def close(self):
        if self.h:
            self.L.amx_histnorm_destroy(self.h)
            self.h = None

    __del__ = close

    def set_scales(self, scales):
        """the scales of training histograms 1 .. n - 1 (the node's `histogram-scale-<i>` ports); histogram 0 gets 1 - their sum"""
        s = np.ascontiguousarray(scales, dtype=np.float32)
        _lib.check(self.L.amx_histnorm_set_scales(self.h, s.ctypes.data))

    def add_key(self, test):
        """the test histograms of one more corpus key -> its number for apply_dev"""
        k = C.c_int()
        _lib.check(self.L.amx_histnorm_add_key(self.h, test.h, C.byref(k)))
        return k.value

    def inverse_cdf(self, d):
        return _lookup_table(self.L.amx_histnorm_inverse_cdf, self.h, int(d))

    def test_cdf(self, key, d):
        return _lookup_table(self.L.amx_histnorm_test_cdf, self.h, int(key), int(d))

    def apply_dev(self, frame_offsets, key_of_segment, in_dev, in_ld, out_dev, out_ld, count_clamped=True):
        """segment s = frames [frame_offsets[s], frame_offsets[s + 1]) with key key_of_segment[s]; in_dev may be out_dev.  Returns
        (clamped at the test CDF, clamped at the inverse CDF), or None without the synchronisation when count_clamped is False."""
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        keys = np.ascontiguousarray(key_of_segment, dtype=np.int32)
        if len(off) != len(keys) + 1:
            raise ValueError("HistogramNormalization.apply_dev: %d frame offsets for %d segments" % (len(off), len(keys)))
        cl = np.zeros(2, np.uint64)
        _lib.check(self.L.amx_histnorm_apply_dev(self.h, len(keys), off.ctypes.data, keys.ctypes.data, _ptr(in_dev), int(in_ld), _ptr(out_dev), int(out_ld),
                                                 cl.ctypes.data if count_clamped else None))
        return (int(cl[0]), int(cl[1])) if count_clamped else None


class BayesClassifier:
    """Signal::BayesClassification with the uniform prior: the decisions of `signal-bayes-classification` (classify) and the vectors of
    `signal-bayes-classification-score` (scores) for a batch of segments whose [frames x classes] score matrix is on the device.
    Keyword names are the fields of amx_bayes_cfg (= the nodes' parameters); ctx None gives a handle for configuration and prior only."""

    def __init__(self, ctx, n_classes, **kw):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        cfg = _lib.BayesCfg()
        self.L.amx_bayes_default_cfg(C.byref(cfg))
        cfg.n_classes = int(n_classes)
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("BayesClassifier: unknown parameter %r" % k)
            setattr(cfg, k, int(v))
        h = C.c_void_p()
        _lib.check(self.L.amx_bayes_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h
        self.n_classes = cfg.n_classes
        self.per_frame = cfg.window_length > 0 or 0 <= cfg.delay < 2 ** 31 - 1

    def close(self):
        if self.h:
            self.L.amx_bayes_destroy(self.h)
            self.h = None

    __del__ = close

    def prior(self):
        """log(n_classes) as the reference's f32 holds it"""
        v = C.c_float()
        _lib.check(self.L.amx_bayes_prior(self.h, C.byref(v)))
        return np.float32(v.value)

    @staticmethod
    def _offsets(frame_offsets):
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise ValueError("BayesClassifier: frame_offsets must hold n_seg + 1 offsets")
        return off

    def classify(self, frame_offsets, scores_dev, scores_ld, segment_label_dev, weights_dev=None, segment_score_dev=None, frame_label_dev=None,
                 sum_of_weights_dev=None, count_no_winner=True):
        """segment s = rows [frame_offsets[s], frame_offsets[s + 1]) of scores_dev.  Fills segment_label_dev (int32 [n_seg]) and the optional
        buffers (amx_bayes_classify_dev); returns (segment labels, frame labels) that are -1 because no class won, or None without the
        synchronisation when count_no_winner is False."""
        off = self._offsets(frame_offsets)
        nw = np.zeros(2, np.uint64)
        _lib.check(self.L.amx_bayes_classify_dev(self.h, len(off) - 1, off.ctypes.data, _ptr(scores_dev), int(scores_ld), _ptr(weights_dev),
                                                 _ptr(segment_label_dev), _ptr(segment_score_dev), _ptr(frame_label_dev), _ptr(sum_of_weights_dev),
                                                 nw.ctypes.data if count_no_winner else None))
        return (int(nw[0]), int(nw[1])) if count_no_winner else None

    def scores(self, frame_offsets, scores_dev, scores_ld, out_dev, out_ld, emitted_dev, weights_dev=None):
        """the score node: row t of out_dev where a vector leaves after frame t (emitted_dev[t] = 1) or, in the segment's last row, at the
        end of the stream (2); other rows keep what they held"""
        off = self._offsets(frame_offsets)
        _lib.check(self.L.amx_bayes_scores_dev(self.h, len(off) - 1, off.ctypes.data, _ptr(scores_dev), int(scores_ld), _ptr(weights_dev), _ptr(out_dev),
                                               int(out_ld), _ptr(emitted_dev)))

    def classify_gmm(self, gmm, frame_offsets, feats_dev, segment_label_dev, weights_dev=None, segment_score_dev=None, frame_label_dev=None,
                     sum_of_weights_dev=None, count_no_winner=True):
        """fast VTLN in one call: gmm (a GmmFeatureScorer of the same context, one mixture per class) scores feats_dev [frames, dim] into a
        matrix the handle owns, then classify"""
        off = self._offsets(frame_offsets)
        nw = np.zeros(2, np.uint64)
        _lib.check(self.L.amx_bayes_classify_gmm_dev(self.h, gmm.h, gmm.mode, len(off) - 1, off.ctypes.data, _ptr(feats_dev), _ptr(weights_dev),
                                                     _ptr(segment_label_dev), _ptr(segment_score_dev), _ptr(frame_label_dev),
                                                     _ptr(sum_of_weights_dev), nw.ctypes.data if count_no_winner else None))
        return (int(nw[0]), int(nw[1])) if count_no_winner else None

    @staticmethod
    def warping_factors(labels, factors):
        """segment labels -> the warping factor of each segment for MfccExtractor.plan (amx_mfcc_plan_create_vtln): class c is the c-th of
        the VTLN handle's factors.  A label of -1 (no frames, no winner) has no factor and raises."""
        labels = np.asarray(labels).astype(np.int64)
        factors = np.asarray(factors, np.float64)
        bad = np.nonzero((labels < 0) | (labels >= len(factors)))[0]
        if len(bad):
            raise ValueError("BayesClassifier.warping_factors: segment %d has label %d, outside the %d factors" % (bad[0], labels[bad[0]], len(factors)))
        return factors[labels]


class StatePosteriorScorer:
    """Mm::StatePosteriorFeatureScorer with viterbi = true on a [frames x mixtures] score matrix that is on the device.  Keyword names are
    the fields of amx_posterior_cfg (= the reference's parameters: scale, pruning_threshold, margin, viterbi); ctx None gives a handle
    for configuration only.  Buffers are device tensors (or anything with data_ptr()); every output is optional."""

    MODES = {"mixture": _lib.AMX_POSTERIOR_MIXTURE, "likelihood": _lib.AMX_POSTERIOR_LIKELIHOOD, "density": _lib.AMX_POSTERIOR_DENSITY}
    OUTPUTS = ("posterior_f32_dev", "posterior_f64_dev", "log_z_dev", "min_dev", "min_index_dev", "n_survivors_dev", "sparse_index_dev",
               "sparse_value_dev", "sparse_count_dev")

    def __init__(self, ctx, n_mixtures, **kw):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        cfg = _lib.PosteriorCfg()
        self.L.amx_posterior_default_cfg(C.byref(cfg))
        cfg.n_mixtures = int(n_mixtures)
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("StatePosteriorScorer: unknown parameter %r" % k)
            setattr(cfg, k, v if isinstance(getattr(cfg, k), float) else int(v))
        h = C.c_void_p()
        _lib.check(self.L.amx_posterior_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h
        self.n_mixtures = cfg.n_mixtures
        self.cfg = cfg

    def close(self):
        if self.h:
            self.L.amx_posterior_destroy(self.h)
            self.h = None

    __del__ = close

    def set_filter(self, mixture, prior=None):
        """the filter: mixtures and their priors (None: 0)"""
        m = np.ascontiguousarray(mixture, dtype=np.int32)
        p = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        if p is not None and len(p) != len(m):
            raise ValueError("StatePosteriorScorer.set_filter: %d priors for %d mixtures" % (len(p), len(m)))
        _lib.check(self.L.amx_posterior_set_filter(self.h, len(m), m.ctypes.data, _ptr(p)))

    def set_default_filter(self):
        _lib.check(self.L.amx_posterior_set_default_filter(self.h))

    def set_single_filter(self, mixture):
        _lib.check(self.L.amx_posterior_set_single_filter(self.h, int(mixture)))

    def set_disregard(self, numbers):
        """disregard-densities: erased from the filter as MIXTURE indices, as the reference does"""
        d = np.ascontiguousarray(numbers, dtype=np.int32)
        _lib.check(self.L.amx_posterior_set_disregard(self.h, len(d), d.ctypes.data if len(d) else None))

    def filter(self):
        """(mixtures, priors) of the filter in effect, in increasing mixture order"""
        n = C.c_int()
        m, p = np.zeros(self.n_mixtures, np.int32), np.zeros(self.n_mixtures, np.float64)
        _lib.check(self.L.amx_posterior_filter(self.h, C.byref(n), m.ctypes.data, p.ctypes.data))
        return m[:n.value].copy(), p[:n.value].copy()

    def set_topology(self, mix_offsets=None, dens_index=None, gmm=None):
        """density-keyed mode: the CSR topology of the mixture set, or that of a GmmFeatureScorer"""
        if gmm is not None:
            _lib.check(self.L.amx_posterior_set_topology_gmm(self.h, gmm.h))
            return
        off = np.ascontiguousarray(mix_offsets, dtype=np.uint32)
        dens = np.ascontiguousarray(dens_index, dtype=np.uint32)
        if len(off) != self.n_mixtures + 1 or (len(off) and len(dens) != int(off[-1])):
            raise ValueError("StatePosteriorScorer.set_topology: mix_offsets must hold n_mixtures + 1 offsets and dens_index mix_offsets[-1] numbers")
        _lib.check(self.L.amx_posterior_set_topology(self.h, off.ctypes.data, dens.ctypes.data))

    def topology_info(self):
        """(monotone, shared density or -1)"""
        mono, shared = C.c_int(), C.c_longlong()
        _lib.check(self.L.amx_posterior_topology_info(self.h, C.byref(mono), C.byref(shared)))
        return bool(mono.value), int(shared.value)

    def _out(self, kw):
        out = _lib.PosteriorOut()
        for k, v in kw.items():
            if k not in self.OUTPUTS and k not in ("posterior_f32_ld", "posterior_f64_ld", "sparse_capacity"):
                raise TypeError("StatePosteriorScorer: unknown output %r" % k)
            setattr(out, k, _ptr(v) if k in self.OUTPUTS else int(v))
        if not out.posterior_f32_ld:
            out.posterior_f32_ld = self.n_mixtures
        if not out.posterior_f64_ld:
            out.posterior_f64_ld = self.n_mixtures
        return out

    def posteriors(self, scores_dev, scores_ld, T, mode="mixture", best_density_dev=None, best_ld=None, margin_mixture_dev=None, count_no_minimum=True,
                   **outputs):
        """amx_posterior_dev: outputs are the fields of amx_posterior_out by name; returns the number of frames without a minimum, or None
        without the synchronisation when count_no_minimum is False"""
        out = self._out(outputs)
        nm = C.c_ulonglong()
        _lib.check(self.L.amx_posterior_dev(self.h, self.MODES[mode], _ptr(scores_dev), int(scores_ld), int(T), _ptr(best_density_dev),
                                            int(best_ld if best_ld is not None else self.n_mixtures), _ptr(margin_mixture_dev), C.byref(out),
                                            C.addressof(nm) if count_no_minimum else None))
        return int(nm.value) if count_no_minimum else None

    def list_posteriors(self, scores_dev, scores_ld, list_offsets, mixture_dev, prior_dev, posterior_f64_dev=None, posterior_f32_dev=None,
                        count_no_minimum=True):
        """amx_posterior_lists_dev: frame t has the candidates [list_offsets[t], list_offsets[t + 1]) of mixture_dev (int32) / prior_dev (f64)"""
        off = np.ascontiguousarray(list_offsets, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise ValueError("StatePosteriorScorer.list_posteriors: list_offsets must hold T + 1 offsets")
        nm = C.c_ulonglong()
        _lib.check(self.L.amx_posterior_lists_dev(self.h, _ptr(scores_dev), int(scores_ld), len(off) - 1, off.ctypes.data, _ptr(mixture_dev), _ptr(prior_dev),
                                                  _ptr(posterior_f64_dev), _ptr(posterior_f32_dev), C.addressof(nm) if count_no_minimum else None))
        return int(nm.value) if count_no_minimum else None

    def posteriors_gmm(self, gmm, feats_dev, T, mode="mixture", margin_mixture_dev=None, count_no_minimum=True, **outputs):
        """gmm (a GmmFeatureScorer of the same context) scores feats_dev [T, dim] into matrices the handle owns, then posteriors"""
        out = self._out(outputs)
        nm = C.c_ulonglong()
        _lib.check(self.L.amx_posterior_gmm_dev(self.h, gmm.h, gmm.mode, self.MODES[mode], _ptr(feats_dev), int(T), _ptr(margin_mixture_dev), C.byref(out),
                                                C.addressof(nm) if count_no_minimum else None))
        return int(nm.value) if count_no_minimum else None

    @staticmethod
    def sort_sparse(index, value, count):
        """the adapter's sort for a topology that is not monotone (StatePosteriorFeatureScorerNode.cc:49-57): host arrays [T, capacity] and
        [T] -> per frame (indices, values) in increasing index order"""
        rows = []
        for t in range(len(count)):
            k = min(int(count[t]), index.shape[1])
            order = np.argsort(index[t, :k], kind="stable")
            rows.append((index[t, :k][order], value[t, :k][order]))
        return rows


class CombinedScorer:
    """Mm::CombinedFeatureScorer: out[t][e] = sum over the models, in model order, of scale[i] * scores[i][t][table[e][i]] in f32.
    table is [n_emissions, n_models]; n_mixtures[i] is the width of model i's matrix.  ctx None validates only."""

    def __init__(self, ctx, n_mixtures, table, scale):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        nm = np.ascontiguousarray(n_mixtures, dtype=np.int32)
        tb = np.ascontiguousarray(table, dtype=np.int32)
        sc = np.ascontiguousarray(scale, dtype=np.float32)
        if tb.ndim != 2 or tb.shape[1] != len(nm) or len(sc) != len(nm):
            raise ValueError("CombinedScorer: table must be [n_emissions, n_models] with one width and one scale per model")
        h = C.c_void_p()
        _lib.check(self.L.amx_combine_create(ctx.h if ctx is not None else None, len(nm), tb.shape[0], nm.ctypes.data, tb.ctypes.data, sc.ctypes.data,
                                             C.byref(h)))
        self.h = h
        self.n_models, self.n_emissions = len(nm), tb.shape[0]

    def close(self):
        if self.h:
            self.L.amx_combine_destroy(self.h)
            self.h = None

    __del__ = close

    def identity_columns(self):
        """per model: whether its table column is 0, 1, 2, ... (read straight)"""
        m = C.c_uint()
        _lib.check(self.L.amx_combine_identity_columns(self.h, C.byref(m)))
        return [bool((m.value >> i) & 1) for i in range(self.n_models)]

    def combine(self, T, scores_dev, ld, out_dev, out_ld):
        """amx_combine_dev: scores_dev is a list of the models' device matrices, ld their leading dimensions"""
        if len(scores_dev) != self.n_models or len(ld) != self.n_models:
            raise ValueError("CombinedScorer.combine: %d models" % self.n_models)
        ptrs = (C.c_void_p * self.n_models)(*[_ptr(s) for s in scores_dev])
        lds = np.ascontiguousarray(ld, dtype=np.int32)
        _lib.check(self.L.amx_combine_dev(self.h, int(T), ptrs, lds.ctypes.data, _ptr(out_dev), int(out_ld)))


def _quanteq_cfg(L, kw, who):
    cfg = _lib.QuanteqCfg()
    L.amx_quanteq_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError("%s: unknown parameter %r" % (who, k))
        setattr(cfg, k, v if isinstance(getattr(cfg, k), float) else int(v))
    return cfg


def _offsets(frame_offsets, who):
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("%s: frame_offsets must hold n_seg + 1 offsets" % who)
    return off


class ViterbiAligner:
    """Search::Aligner in Viterbi mode (what Speech::AlignmentNode runs) for a batch of segments whose [frames x emissions] score matrix
    is on the device.  Keyword names are the fields of amx_align_cfg (= the aligner's parameters); ctx None gives a handle that only
    checks configurations and graphs."""

    FLOATS = ("min_acoustic_pruning", "max_acoustic_pruning", "increment_factor", "min_average_number_of_states", "score_scale")

    def __init__(self, ctx, **kw):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        cfg = _lib.AlignCfg()
        self.L.amx_align_default_cfg(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("ViterbiAligner: unknown parameter %r" % k)
            setattr(cfg, k, float(v) if k in self.FLOATS else int(v))
        h = C.c_void_p()
        _lib.check(self.L.amx_align_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.L.amx_align_destroy(self.h)
            self.h = None

    __del__ = close

    @staticmethod
    def graphs(segments):
        """the host tables of amx_align_graphs from one dict per segment: n_states, initial, final (bool per state), final_weight (per
        state) and arcs, a list per source state of (target, emission, label, weight) in the reference's arc order.  Returns a dict of
        numpy arrays named like the struct's fields."""
        state_offsets, arc_offsets = [0], [0]
        initial, is_final, final_weight, target, emission, label, weight = [], [], [], [], [], [], []
        for g in segments:
            n = int(g["n_states"])
            if len(g["arcs"]) != n or len(g["final"]) != n or len(g["final_weight"]) != n:
                raise ValueError("ViterbiAligner.graphs: a segment's tables do not have n_states entries")
            state_offsets.append(state_offsets[-1] + n)
            initial.append(int(g["initial"]))
            is_final.extend(bool(f) for f in g["final"])
            final_weight.extend(float(w) for w in g["final_weight"])
            for arcs in g["arcs"]:
                for t, e, l, w in arcs:
                    target.append(int(t)), emission.append(int(e)), label.append(int(l)), weight.append(float(w))
                arc_offsets.append(len(target))
        return dict(state_offsets=np.array(state_offsets, np.int32), initial_state=np.array(initial, np.int32), is_final=np.array(is_final, np.uint8),
                    final_weight=np.array(final_weight, np.float32), arc_offsets=np.array(arc_offsets, np.int32), arc_target=np.array(target, np.int32),
                    arc_emission=np.array(emission, np.int32), arc_label=np.array(label, np.int32), arc_weight=np.array(weight, np.float32))

    def align(self, frame_offsets, graphs, scores_dev, scores_ld, n_columns=None, label_dev=None, emission_dev=None, arc_score_dev=None):
        """segment s = rows [frame_offsets[s], frame_offsets[s + 1]) of scores_dev.  graphs: what graphs() returns, or the list it takes.
        label_dev, emission_dev (int32) and arc_score_dev (f32) hold one entry per row of the matrix up to frame_offsets[-1]; buffers
        that are not given are created (torch, on the matrix's device).  Returns (label_dev, emission_dev, arc_score_dev, results,
        counters): results is a list of dicts per segment, counters (segments that met a NaN, passes run, passes counted)."""
        off = _offsets(frame_offsets, "ViterbiAligner.align")
        if not isinstance(graphs, dict):
            graphs = self.graphs(graphs)
        n_seg = len(off) - 1
        if len(graphs["state_offsets"]) != n_seg + 1:
            raise ValueError("ViterbiAligner.align: %d segments but graphs of %d" % (n_seg, len(graphs["state_offsets"]) - 1))
        keep = {k: np.ascontiguousarray(v) for k, v in graphs.items()}
        g = _lib.AlignGraphs(**{k: v.ctypes.data for k, v in keep.items()})
        if self.ctx is not None and int(off[-1]) > 0:
            import torch
            if label_dev is None:
                label_dev = torch.empty(int(off[-1]), dtype=torch.int32, device=scores_dev.device)
            if emission_dev is None:
                emission_dev = torch.empty(int(off[-1]), dtype=torch.int32, device=scores_dev.device)
            if arc_score_dev is None:
                arc_score_dev = torch.empty(int(off[-1]), dtype=torch.float32, device=scores_dev.device)
        res = (_lib.AlignResult * max(n_seg, 1))()
        counters = np.zeros(3, np.uint64)
        _lib.check(self.L.amx_align_viterbi_dev(self.h, n_seg, off.ctypes.data, C.byref(g), _ptr(scores_dev), int(scores_ld),
                                                int(n_columns if n_columns is not None else scores_ld), _ptr(label_dev), _ptr(emission_dev),
                                                _ptr(arc_score_dev), C.cast(res, C.c_void_p), counters.ctypes.data))
        results = [dict(score=np.float32(r.score), reached=bool(r.reached_final), n_iterations=int(r.n_iterations),
                        last_threshold=np.float32(r.last_threshold), average_states=float(r.average_states), state_sum=int(r.state_sum))
                   for r in res[:n_seg]]
        return label_dev, emission_dev, arc_score_dev, results, tuple(int(c) for c in counters)


class LinearSegmenter:
    """Speech::LinearSegmenter (the node speech-linear-segmentation) for a batch of segments whose energy is a column of a feature matrix on
    the device: the first alignment of a training, made without a model.  Keyword names are the fields of amx_linseg_cfg (= the
    segmenter's and its delimiter's parameters); ctx None gives a handle that only checks configurations and segment tables."""

    FLOATS = ("penalty", "minimum_speech_proportion")
    REASONS = ("ok", "too_short", "too_long", "no_states", "jump", "mismatch", "nonfinite")

    def __init__(self, ctx, **kw):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        cfg = _lib.LinsegCfg()
        self.L.amx_linseg_default_cfg(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("LinearSegmenter: unknown parameter %r" % k)
            setattr(cfg, k, float(v) if k in self.FLOATS else int(v))
        h = C.c_void_p()
        _lib.check(self.L.amx_linseg_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.L.amx_linseg_destroy(self.h)
            self.h = None

    __del__ = close

    @staticmethod
    def models(segments, silence_label, silence_emission):
        """the host tables of amx_linseg_models from one (labels, emissions) pair per segment: the flat model's allophone-state ids in
        path order and the emission index of each.  Returns a dict named like the struct's fields."""
        offsets, label, emission = [0], [], []
        for lab, emi in segments:
            if len(lab) != len(emi):
                raise ValueError("LinearSegmenter.models: %d labels but %d emission indices" % (len(lab), len(emi)))
            label.extend(int(v) for v in lab), emission.extend(int(v) for v in emi)
            offsets.append(len(label))
        return dict(state_offsets=np.array(offsets, np.int32), state_label=np.array(label, np.int32), state_emission=np.array(emission, np.int32),
                    silence_label=int(silence_label), silence_emission=int(silence_emission))

    def align(self, frame_offsets, models, energy_dev, energy_ld=1, label_dev=None, emission_dev=None):
        """segment s = rows [frame_offsets[s], frame_offsets[s + 1]); the energy of row t is energy_dev[t * energy_ld] (f32, on the device:
        a column of a feature matrix with energy_ld its row length).  models: what models() returns.  label_dev and emission_dev (int32)
        hold one entry per row up to frame_offsets[-1]; buffers that are not given are created (torch, on the energies' device).
        Returns (label_dev, emission_dev, results, counters): results a list of dicts per segment (reason, its name, speech_begin,
        speech_end, score), counters the segments by reason."""
        off = _offsets(frame_offsets, "LinearSegmenter.align")
        n_seg = len(off) - 1
        if len(models["state_offsets"]) != n_seg + 1:
            raise ValueError("LinearSegmenter.align: %d segments but models of %d" % (n_seg, len(models["state_offsets"]) - 1))
        keep = {k: np.ascontiguousarray(models[k], np.int32) for k in ("state_offsets", "state_label", "state_emission")}
        m = _lib.LinsegModels(keep["state_offsets"].ctypes.data, keep["state_label"].ctypes.data, keep["state_emission"].ctypes.data,
                              int(models["silence_label"]), int(models["silence_emission"]))
        if self.ctx is not None and int(off[-1]) > 0:
            import torch
            if label_dev is None:
                label_dev = torch.empty(int(off[-1]), dtype=torch.int32, device=energy_dev.device)
            if emission_dev is None:
                emission_dev = torch.empty(int(off[-1]), dtype=torch.int32, device=energy_dev.device)
        res = (_lib.LinsegResult * max(n_seg, 1))()
        counters = np.zeros(_lib.AMX_LINSEG_N_REASONS, np.uint64)
        _lib.check(self.L.amx_linseg_align_dev(self.h, n_seg, off.ctypes.data, C.byref(m), _ptr(energy_dev), int(energy_ld), _ptr(label_dev),
                                               _ptr(emission_dev), C.cast(res, C.c_void_p), counters.ctypes.data))
        results = [dict(reason=int(r.reason), reason_name=self.REASONS[r.reason], speech_begin=int(r.speech_begin), speech_end=int(r.speech_end),
                        score=float(r.score)) for r in res[:n_seg]]
        return label_dev, emission_dev, results, tuple(int(c) for c in counters)

    def chains(self, segment, frames):
        """debug: M_ and Q_ (frames + 1 doubles each) of a segment of the last call, read from the handle's workspace"""
        m, q = np.zeros(frames + 1, np.float64), np.zeros(frames + 1, np.float64)
        _lib.check(self.L.amx_linseg_chains(self.h, int(segment), m.ctypes.data, q.ctypes.data))
        return m, q


class CartExampleAccumulator:
    """Speech::FeatureAccumulator on the device: one Cart::Example per allophone state, row id = [nObs, sum[dim], sumSq[dim]] of one flat f64
    device buffer [n_labels x (1 + 2 dim)] (`acc`, a torch tensor that ranks may all-reduce).  Feed the aligned corpus in order, cut into
    calls anywhere: every (label, component) is one chain over the frames in ascending order that continues across calls."""

    def __init__(self, ctx, n_labels, dim):
        import torch
        self.L, self.ctx, self.n_labels, self.dim = _lib.lib(), ctx, int(n_labels), int(dim)
        size = int(self.L.amx_cart_accumulator_size(self.n_labels, self.dim))
        if size == 0:
            raise ValueError("CartExampleAccumulator: n_labels %d, dim %d" % (self.n_labels, self.dim))
        self.acc = torch.zeros(size, dtype=torch.float64, device="cuda:%d" % ctx.device)

    def accumulate(self, feats_dev, label_dev, weight_dev=None, feats_stride=None):
        """feats_dev [T x dim] f32 (or rows feats_stride floats apart), label_dev [T] int32 as the aligners leave it (-1: skipped),
        weight_dev [T] f64 or None (weight 1)"""
        T = int(label_dev.shape[0])
        stride = int(feats_stride) if feats_stride is not None else (int(feats_dev.stride(0)) if feats_dev.dim() == 2 else self.dim)
        _lib.check(self.L.amx_cart_accumulate_dev(self.ctx.h, _ptr(feats_dev), stride, self.dim, T, _ptr(label_dev), _ptr(weight_dev), self.n_labels,
                                                  _ptr(self.acc)))

    def rows(self):
        """the accumulator on the host, [n_labels x (1 + 2 dim)]"""
        return self.acc.cpu().numpy().reshape(self.n_labels, 1 + 2 * self.dim)

    def examples(self):
        """(ids, n_obs, values) of the labels that were seen: what DecisionTreeTrainer.train takes"""
        r = self.rows()
        ids = np.nonzero(r[:, 0] != 0)[0]
        return ids, np.ascontiguousarray(r[ids, 0]), np.ascontiguousarray(r[ids, 1:])


class DecisionTreeTrainer:
    """Cart::DecisionTreeTrainer with StateTyingDecisionTreeTrainer::LogLikelihoodGain: the sums of every (node, question) on the device,
    the tree logic as the reference writes it.  The questions stay with the caller: `answers` holds question(properties of example) == TRUE
    for every question and example, as a bool matrix [Q x E] or packed by pack_answers."""

    ACTIONS = {"split": _lib.AMX_CART_SPLIT, "partition": _lib.AMX_CART_PARTITION, "cluster": _lib.AMX_CART_CLUSTER}

    def __init__(self, ctx, max_leaves=0xffffffff, variance_clipping=0.0, exact_all=False):
        self.L, self.ctx = _lib.lib(), ctx
        self.max_leaves, self.variance_clipping, self.exact_all = int(max_leaves), float(variance_clipping), bool(exact_all)

    @staticmethod
    def pack_answers(answers):
        """bool [Q x E] -> uint32 [Q x ceil(E / 32)], bit (e & 31) of word e // 32"""
        a = np.asarray(answers, dtype=bool)
        q, e = a.shape
        pad = np.zeros((q, (e + 31) // 32 * 32), np.uint8)
        pad[:, :e] = a
        return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view("<u4"))

    @staticmethod
    def kernel_shape(dim):
        """(examples per LDS stage, questions per workgroup) of the split search for this dimension"""
        s, q = C.c_int(), C.c_int()
        _lib.lib().amx_cart_kernel_shape(int(dim), C.addressof(s), C.addressof(q))
        return s.value, q.value

    def train(self, n_obs, values, answers, steps):
        """n_obs [E] f64, values [E x 2 dim] f64 (sum, then sumSq), answers as above; steps: dicts with action ("split" | "partition" |
        "cluster"), questions (rows of answers), and optionally min_obs, min_gain, randomize.  Returns a dict: nodes (in `order`), classes,
        log, question_stats (structured arrays) and the fields of amx_cart_info."""
        n_obs = np.ascontiguousarray(n_obs, np.float64)
        values = np.ascontiguousarray(values, np.float64)
        E = len(n_obs)
        if values.ndim != 2 or values.shape[0] != E or values.shape[1] % 2:
            raise ValueError("DecisionTreeTrainer.train: values must be [%d x 2 dim]" % E)
        answers = np.asarray(answers)
        bits = self.pack_answers(answers) if answers.dtype == bool else np.ascontiguousarray(answers, np.uint32)
        if bits.ndim != 2 or bits.shape[1] != (E + 31) // 32:
            raise ValueError("DecisionTreeTrainer.train: answers must be [Q x %d] words" % ((E + 31) // 32))
        keep, arr = [], (_lib.CartStep * max(len(steps), 1))()
        for i, st in enumerate(steps):
            unknown = set(st) - {"action", "questions", "min_obs", "min_gain", "randomize"}
            if unknown:
                raise TypeError("DecisionTreeTrainer.train: step %d: unknown field %r" % (i, sorted(unknown)[0]))
            q = np.ascontiguousarray(st["questions"], np.int32)
            keep.append(q)
            action = self.ACTIONS.get(st["action"], st["action"]) if isinstance(st["action"], str) else st["action"]
            if isinstance(action, str):
                raise ValueError("DecisionTreeTrainer.train: step %d: unknown action %r" % (i, action))
            arr[i] = _lib.CartStep(int(action), int(st.get("min_obs", 0)), float(st.get("min_gain", 0.0)), int(st.get("randomize", 1)), len(q), q.ctypes.data)
        pb = _lib.CartProblem(E, values.shape[1] // 2, bits.shape[0], n_obs.ctypes.data, values.ctypes.data, bits.ctypes.data)
        plan = _lib.CartPlan(self.max_leaves, len(steps), C.cast(arr, C.c_void_p), self.variance_clipping, int(self.exact_all))
        h = C.c_void_p()
        _lib.check(self.L.amx_cart_train(self.ctx.h if self.ctx is not None else None, C.byref(pb), C.byref(plan), C.byref(h)))
        try:
            info = _lib.CartInfo()
            _lib.check(self.L.amx_cart_tree_info(h, C.byref(info)))
            nodes = np.zeros(info.n_nodes, np.dtype(_lib.CartNode))
            classes = np.zeros(info.n_examples, np.int32)
            log = np.zeros(info.n_commits, np.dtype(_lib.CartCommit))
            qstats = np.zeros(info.n_question_stats, np.dtype(_lib.CartQstat))
            _lib.check(self.L.amx_cart_tree_get(h, nodes.ctypes.data, classes.ctypes.data, log.ctypes.data, qstats.ctypes.data))
        finally:
            self.L.amx_cart_tree_destroy(h)
        out = dict(nodes=nodes, classes=classes, log=log, question_stats=qstats)
        out.update({k: getattr(info, k) for k, _ in _lib.CartInfo._fields_})
        return out


class BaumWelchAligner:
    """Search::Aligner in mode baum-welch for a batch of segments whose [frames x emissions] score matrix is on the device: forward
    search with pruning, f64 forward-backward over the survivors, and per frame the list of (label, emission index, posterior weight).
    Keyword names are the fields of amx_bw_cfg; ctx None gives a handle that only checks configurations and graphs."""

    FLOATS = ("min_acoustic_pruning", "max_acoustic_pruning", "increment_factor", "min_average_number_of_states", "score_scale", "min_weight")
    graphs = staticmethod(ViterbiAligner.graphs)

    def __init__(self, ctx, **kw):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        cfg = _lib.BwCfg()
        self.L.amx_bw_default_cfg(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("BaumWelchAligner: unknown parameter %r" % k)
            setattr(cfg, k, float(v) if k in self.FLOATS else int(v))
        h = C.c_void_p()
        _lib.check(self.L.amx_bw_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.L.amx_bw_destroy(self.h)
            self.h = None

    __del__ = close

    def align(self, frame_offsets, graphs, scores_dev, scores_ld, n_columns=None, item_offsets_dev=None, weight_f64=True):
        """segment s = rows [frame_offsets[s], frame_offsets[s + 1]) of scores_dev.  graphs: what graphs() returns, or the list it takes.
        Returns (items, item_offsets_dev, results, counters): items is a dict of device tensors frame, label, emission (int32), weight
        (f32) and weight_f64 (None when not asked for), ordered by frame, then decreasing weight, then label; item_offsets_dev (int64,
        one entry per matrix row up to frame_offsets[-1], plus one) says where a row's items lie; results is a list of dicts per segment."""
        off = _offsets(frame_offsets, "BaumWelchAligner.align")
        if not isinstance(graphs, dict):
            graphs = self.graphs(graphs)
        n_seg = len(off) - 1
        if len(graphs["state_offsets"]) != n_seg + 1:
            raise ValueError("BaumWelchAligner.align: %d segments but graphs of %d" % (n_seg, len(graphs["state_offsets"]) - 1))
        keep = {k: np.ascontiguousarray(v) for k, v in graphs.items()}
        g = _lib.AlignGraphs(**{k: v.ctypes.data for k, v in keep.items()})
        torch = None
        if self.ctx is not None:
            import torch
            if item_offsets_dev is None:
                item_offsets_dev = torch.zeros(int(off[-1]) + 1, dtype=torch.int64, device=scores_dev.device)
        res = (_lib.BwResult * max(n_seg, 1))()
        counters = np.zeros(3, np.uint64)
        _lib.check(self.L.amx_bw_align_dev(self.h, n_seg, off.ctypes.data, C.byref(g), _ptr(scores_dev), int(scores_ld),
                                           int(n_columns if n_columns is not None else scores_ld), _ptr(item_offsets_dev), C.cast(res, C.c_void_p),
                                           counters.ctypes.data))
        results = [dict(score=np.float32(r.score), reached=bool(r.reached_final), n_iterations=int(r.n_iterations),
                        last_threshold=np.float32(r.last_threshold), average_states=float(r.average_states), state_sum=int(r.state_sum),
                        n_items=int(r.n_items), log_total=float(r.log_total))
                   for r in res[:n_seg]]
        items = self.items(scores_dev.device, weight_f64) if self.ctx is not None else None
        return items, item_offsets_dev, results, tuple(int(c) for c in counters)

    def items(self, device, weight_f64=True, capacity=None):
        """the item list of the last align() as device tensors of `capacity` (default: the number of items) entries"""
        import torch
        n = int(self.L.amx_bw_n_items(self.h))
        cap = n if capacity is None else int(capacity)
        out = dict(frame=torch.empty(cap, dtype=torch.int32, device=device), label=torch.empty(cap, dtype=torch.int32, device=device),
                   emission=torch.empty(cap, dtype=torch.int32, device=device), weight=torch.empty(cap, dtype=torch.float32, device=device),
                   weight_f64=torch.empty(cap, dtype=torch.float64, device=device) if weight_f64 else None)
        _lib.check(self.L.amx_bw_items_dev(self.h, cap, _ptr(out["frame"]), _ptr(out["label"]), _ptr(out["emission"]), _ptr(out["weight"]),
                                           _ptr(out["weight_f64"])))
        return out


def gather_rows(ctx, src_dev, row_dev, dst_dev=None):
    """dst[i] = src[row_dev[i]] for an f32 matrix and int32 row numbers on the device (amx_gather_rows_dev)"""
    import torch
    n, dim = int(row_dev.numel()), int(src_dev.shape[1])
    if dst_dev is None:
        dst_dev = torch.empty((n, dim), dtype=torch.float32, device=src_dev.device)
    _lib.check(_lib.lib().amx_gather_rows_dev(ctx.h, _ptr(src_dev), int(src_dev.stride(0)), dim, n, _ptr(row_dev), _ptr(dst_dev), int(dst_dev.stride(0))))
    return dst_dev


def read_quantiles(path, dim, number_of_quantiles=4, pool=True):
    """the training quantile file of `signal-quantile-equalization` -> f32 [(nq + 1), dim]; pool: each quantile averaged over the channels"""
    out = np.zeros((int(number_of_quantiles) + 1, int(dim)), np.float32)
    _lib.check(_lib.lib().amx_quanteq_quantiles_read(os.fsencode(path), int(dim), int(number_of_quantiles), int(bool(pool)), out.ctypes.data))
    return out


def write_quantiles(path, sums, count):
    """the file the node writes in estimation mode: sums f64 [(nq + 1), dim] divided by count"""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    _lib.check(_lib.lib().amx_quanteq_quantiles_write(os.fsencode(path), s.shape[1], s.shape[0] - 1, s.ctypes.data, int(count)))


class QuantileEqualization:
    """Signal::QuantileEqualization in segment mode: quantiles, the alpha / gamma (and lambda / rho) grid search, the power function and
    joint mean / variance normalisation for a batch of segments in one call.  Keyword names are the fields of amx_quanteq_cfg (= the
    node's parameters); training_quantiles is what read_quantiles returns; ctx None gives a handle for configuration and grids only."""

    def __init__(self, ctx, dim, training_quantiles=None, **kw):
        self.L, self.h = _lib.lib(), None
        self.ctx = ctx
        cfg = _quanteq_cfg(self.L, kw, type(self).__name__)
        self._configure(cfg)
        tq = None
        if training_quantiles is not None:
            tq = np.ascontiguousarray(training_quantiles, dtype=np.float32)
            if tq.shape != (cfg.number_of_quantiles + 1, int(dim)):
                raise ValueError("%s: training_quantiles has shape %s, not %s" % (type(self).__name__, tq.shape, (cfg.number_of_quantiles + 1, int(dim))))
        h = C.c_void_p()
        _lib.check(self.L.amx_quanteq_create(ctx.h if ctx is not None else None, int(dim), C.byref(cfg), _ptr(tq), C.byref(h)))
        self.h = h
        self.dim, self.nq = int(dim), cfg.number_of_quantiles

    def _configure(self, cfg):
        if cfg.estimate:
            raise TypeError("QuantileEqualization: estimate = 1 is QuantileEstimator")

    def close(self):
        if self.h:
            self.L.amx_quanteq_destroy(self.h)
            self.h = None

    __del__ = close

    def grid(self, which):
        """the grid the search walks: "alpha", "gamma" or "lambda" (also rho's)"""
        k = {"alpha": 0, "gamma": 1, "lambda": 2, "rho": 2}[which]
        n = C.c_int()
        _lib.check(self.L.amx_quanteq_grid(self.h, k, C.byref(n), None))
        v = np.zeros(n.value, np.float32)
        _lib.check(self.L.amx_quanteq_grid(self.h, k, C.byref(n), v.ctypes.data))
        return v

    def apply_dev(self, frame_offsets, in_dev, in_ld, out_dev, out_ld, want_params=False):
        """segment s = rows [frame_offsets[s], frame_offsets[s + 1]); out_dev may be in_dev.  With want_params returns a dict of
        alpha, gamma, lambda, rho, mean, deviation [n_seg, dim] and quantiles [n_seg, nq + 1, dim] (as first taken)."""
        off = _offsets(frame_offsets, "QuantileEqualization.apply_dev")
        n_seg = len(off) - 1
        par = np.zeros((n_seg, 6 + self.nq + 1, self.dim), np.float32) if want_params else None
        _lib.check(self.L.amx_quanteq_apply_dev(self.h, n_seg, off.ctypes.data, _ptr(in_dev), int(in_ld), _ptr(out_dev), int(out_ld), _ptr(par)))
        if not want_params:
            return None
        out = {name: par[:, k] for k, name in enumerate(("alpha", "gamma", "lambda", "rho", "mean", "deviation"))}
        out["quantiles"] = par[:, 6:]
        return out


class QuantileEstimator(QuantileEqualization):
    """the node with estimate = true: the quantiles of every segment, taken on the device, summed on the host in segment order"""

    def __init__(self, ctx, dim, **kw):
        super().__init__(ctx, dim, None, estimate=1, **kw)

    def _configure(self, cfg):
        pass

    def apply_dev(self, *a, **kw):
        raise TypeError("QuantileEstimator: the output stream of estimation mode is not built")

    def accumulate_dev(self, frame_offsets, in_dev, in_ld):
        off = _offsets(frame_offsets, "QuantileEstimator.accumulate_dev")
        _lib.check(self.L.amx_quanteq_estimate_dev(self.h, len(off) - 1, off.ctypes.data, _ptr(in_dev), int(in_ld)))

    def result(self):
        """(sums f64 [nq + 1, dim], count)"""
        sums = np.zeros((self.nq + 1, self.dim), np.float64)
        n = C.c_ulonglong()
        _lib.check(self.L.amx_quanteq_estimate_result(self.h, sums.ctypes.data, C.byref(n)))
        return sums, n.value

    def write(self, path):
        sums, n = self.result()
        write_quantiles(path, sums, n)


def layer_from_parameters(params, has_bias=True):
    """parameter matrix [out, has_bias + in] (column 0 = bias) -> (W [out, in], bias [out])"""
    p = np.ascontiguousarray(params, dtype=np.float32)
    out, cols = p.shape
    W = np.zeros((out, cols - int(has_bias)), np.float32)
    b = np.zeros(out, np.float32)
    _lib.check(_lib.lib().amx_nn_layer_from_parameters(p.ctypes.data, out, cols, int(has_bias), W.ctypes.data, b.ctypes.data))
    return W, b


def prior_from_mixture_set(model):
    """Nn::Prior::setFromMixtureSet: log prior per mixture from the mixture weights"""
    keep = []
    st = _gmm_struct(model, 1.0, 1.0, keep)
    out = np.zeros(st.n_mix, np.float32)
    _lib.check(_lib.lib().amx_prior_from_mixture_set(C.byref(st), out.ctypes.data))
    return out


class FeedForwardTrainer:
    """Nn::FeedForwardTrainer in batch mode and Nn::MeanAndVarianceTrainer: the statistics pass over aligned frames into ONE flat f64
    accumulator (include/amx.h, "NN training statistics").  Ws[l] is [out, in] as NnBatchFeatureScorer takes it; Ws=None builds no
    network (class counts and mean and variance only; give feature_dim / n_outputs).  ctx may be None for host-only use (files, prior,
    mean and deviation)."""

    FLAGS = {"class-counts": _lib.AMX_NNSTAT_CLASS_COUNTS, "mean-and-variance": _lib.AMX_NNSTAT_MEAN_AND_VARIANCE,
             "base": _lib.AMX_NNSTAT_BASE, "gradient": _lib.AMX_NNSTAT_GRADIENT}

    def __init__(self, ctx, Ws=None, biases=None, activations=None, statistics=("base", "gradient"), error_signal_clip=None, class_weights=None,
                 class_to_output=None, preprocessing=None, maxout=None, feature_dim=0, n_outputs=0, precision="fp32"):
        self.ctx, self.L = ctx, _lib.lib()
        mask = statistics if isinstance(statistics, int) else sum(self.FLAGS[s] for s in set(statistics))
        cfg = _lib.NnTrainCfg()
        self.L.amx_nntrain_default_cfg(C.byref(cfg))
        cfg.statistics = mask
        if error_signal_clip is not None:
            cfg.error_signal_clip = error_signal_clip
        self._cw = None if class_weights is None else np.ascontiguousarray(class_weights, dtype=np.float32)
        self._map = None if class_to_output is None else np.ascontiguousarray(class_to_output, dtype=np.int32)
        cfg.class_weights = _ptr(self._cw)
        h = C.c_void_p()
        if Ws is None:
            cfg.feature_dim, cfg.n_outputs = int(feature_dim), int(n_outputs)
            cfg.n_classes, cfg.class_to_output = (0 if self._map is None else len(self._map)), _ptr(self._map)
            expect = cfg.n_outputs
            model = ext = None
        else:
            n = len(Ws)
            self._Ws = [np.ascontiguousarray(w, dtype=np.float32) for w in Ws]
            self._bs = [np.ascontiguousarray(b, dtype=np.float32) for b in biases]
            self._ind = np.array([w.shape[1] for w in self._Ws], np.int32)
            self._outd = np.array([w.shape[0] for w in self._Ws], np.int32)
            self._act = np.array(activations, np.int32)
            Wp = (C.c_void_p * n)(*[w.ctypes.data for w in self._Ws])
            Bp = (C.c_void_p * n)(*[b.ctypes.data for b in self._bs])
            st = _lib.FfnnModel(n, self._ind.ctypes.data, self._outd.ctypes.data, C.cast(Wp, C.c_void_p), C.cast(Bp, C.c_void_p), self._act.ctypes.data,
                                None, 0.0, {"fp32": AMX_PREC_FP32, "bf16": AMX_PREC_BF16, "bf16x3": _lib.AMX_PREC_BF16X3, "f16mx": _lib.AMX_PREC_F16MX}[precision],
                                0 if self._map is None else len(self._map), _ptr(self._map), None)
            model = C.byref(st)
            ext = None
            if preprocessing or maxout:
                self._ext = NnBatchFeatureScorer._layers(self, n, preprocessing or [], maxout or {})
                ext = C.byref(self._ext)
            expect = int(self._outd[-1])
        if self._cw is not None and len(self._cw) != expect:
            raise ValueError("class_weights has %d entries, the network %d outputs" % (len(self._cw), expect))
        _lib.check(self.L.amx_nntrain_create(None if ctx is None else ctx.h, model, ext, C.byref(cfg), C.byref(h)))
        self.h = h
        self.mask = mask
        lay = _lib.NnTrainLayout()
        _lib.check(self.L.amx_nntrain_layout(h, C.byref(lay)))
        self.layout = lay
        self.n_layers, self.feature_dim, self.n_outputs = lay.n_layers, lay.feature_dim, lay.n_outputs

    def close(self):
        if getattr(self, "h", None):
            self.L.amx_nntrain_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulator_size(self):
        return int(self.L.amx_nntrain_accumulator_size(self.h))

    def accumulate_dev(self, feats_dev, feats_stride, T, emission_dev, acc_dev, weight_dev=None):
        """one mini-batch of at most AMX_NNTRAIN_MAX_FRAMES frames: feats_dev f32 [T x feats_stride], emission_dev u32 [T] class
        indices (the aligners' emission_dev), weight_dev f64 [T] or None, acc_dev f64 [accumulator_size()]"""
        if self.ctx is None:
            raise RuntimeError("FeedForwardTrainer.accumulate_dev: created without a context")
        _lib.check(self.L.amx_nntrain_accumulate_dev(self.h, _ptr(feats_dev), int(feats_stride), int(T), _ptr(emission_dev), _ptr(weight_dev), _ptr(acc_dev)))

    def accumulate(self, feats, emission, acc_dev, weights=None):
        """the same for numpy arrays or device tensors of any length: numpy inputs are uploaded, and the frames go through
        accumulate_dev in slices of AMX_NNTRAIN_MAX_FRAMES (the buffer adds up)"""
        import torch
        dev = "cuda:%d" % self.ctx.device if hasattr(self.ctx, "device") else "cuda"

        def up(a, dtype, view=None):
            if a is None or hasattr(a, "data_ptr"):
                return a
            a = np.ascontiguousarray(a, dtype=dtype)
            return torch.from_numpy(a if view is None else a.view(view)).to(dev)
        f, e, w = up(feats, np.float32), up(emission, np.uint32, np.int32), up(weights, np.float64)
        T, ld = int(f.shape[0]), int(f.stride(0))
        step = _lib.AMX_NNTRAIN_MAX_FRAMES
        torch.cuda.synchronize()   # the uploads and the caller's buffer are torch's work, the pass runs on the context's stream
        for t0 in range(0, T, step):
            n = min(step, T - t0)
            self.accumulate_dev(f[t0:], ld, n, None if e is None else e[t0:], acc_dev, None if w is None else w[t0:])
        self.ctx.synchronize()

    def _host(self, acc):
        if not isinstance(acc, np.ndarray):
            acc = acc.detach().cpu().numpy()
        a = np.ascontiguousarray(acc, dtype=np.float64)
        if a.size != self.accumulator_size():
            raise ValueError("accumulator has %d entries, expected %d" % (a.size, self.accumulator_size()))
        return a

    def statistics(self, acc):
        """the blocks of a flat accumulator (device tensor or numpy) as a dict: n_observations, n_classification_errors, total_weight,
        objective; class_counts [n_outputs]; feature_sum, feature_square_sum [feature_dim]; gradient_weights (per layer [in, out], the
        file's order) and gradient_bias (per layer [out]) -- those the handle's statistics hold"""
        a, y = self._host(acc), self.layout
        d = {"n_observations": int(a[y.tail]), "n_classification_errors": int(a[y.tail + 1]), "total_weight": float(a[y.tail + 2]),
             "objective": float(a[y.tail + 3])}
        if y.class_counts >= 0:
            d["class_counts"] = a[y.class_counts:y.class_counts + y.n_outputs].astype(np.int64)
        if y.feature_sum >= 0:
            d["feature_sum"] = a[y.feature_sum:y.feature_sum + y.feature_dim].copy()
            d["feature_square_sum"] = a[y.feature_square_sum:y.feature_square_sum + y.feature_dim].copy()
        if self.mask & _lib.AMX_NNSTAT_GRADIENT:
            d["gradient_weights"] = [a[y.gradient_weights[l]:y.gradient_weights[l] + y.in_dim[l] * y.out_dim[l]].reshape(y.in_dim[l], y.out_dim[l]).copy()
                                     for l in range(y.n_layers)]
            d["gradient_bias"] = [a[y.gradient_bias[l]:y.gradient_bias[l] + y.out_dim[l]].copy() for l in range(y.n_layers)]
        return d

    def write(self, acc, path):
        """flat accumulator -> Nn::Statistics<f32> file (`statistics-filename`), narrowed to single precision"""
        a = self._host(acc)
        _lib.check(self.L.amx_nnstat_write(self.h, a.ctypes.data, os.fsencode(path)))

    def read(self, path):
        """Nn::Statistics<f32> file of this handle's statistics and shapes -> flat accumulator (numpy f64)"""
        a = np.zeros(self.accumulator_size(), np.float64)
        _lib.check(self.L.amx_nnstat_read(self.h, os.fsencode(path), a.ctypes.data))
        return a


class MiniBatchTrainer(FeedForwardTrainer):
    """Nn::FeedForwardTrainer with batch-mode = false and Nn::BatchEstimator (include/amx.h, "NN mini-batch training"): the statistics
    pass of FeedForwardTrainer into the handle's own single-precision statistics, the regulariser, finalize and the estimator's step
    on the device.  The statistics are always base + gradient."""

    REGULARIZERS = {None: _lib.AMX_NNSTEP_REG_NONE, "none": _lib.AMX_NNSTEP_REG_NONE, "l1": _lib.AMX_NNSTEP_REG_L1, "l2": _lib.AMX_NNSTEP_REG_L2,
                    "centered-l2": _lib.AMX_NNSTEP_REG_CENTERED_L2}
    SMOOTHING = {None: _lib.AMX_NNSTEP_STAT_NO_STATISTICS, "no-statistics": _lib.AMX_NNSTEP_STAT_NO_STATISTICS, "none": _lib.AMX_NNSTEP_STAT_NONE,
                 "exponential-trace": _lib.AMX_NNSTEP_STAT_EXPONENTIAL_TRACE}
    ESTIMATORS = {"mean-normalized-sgd": _lib.AMX_NNSTEP_MEAN_NORMALIZED_SGD,
                  "mean-normalized-sgd-l1-clipping": _lib.AMX_NNSTEP_MEAN_NORMALIZED_SGD_L1_CLIPPING}

    def __init__(self, ctx, Ws, biases, activations, **kw):
        kw.setdefault("statistics", ("base", "gradient"))
        super().__init__(ctx, Ws, biases, activations, **kw)

    def set_estimator(self, learning_rate=1.0, bias_learning_rate=1.0, layer_learning_rate=None, regularization_constant=None, trainable=None,
                      regularizer=None, center=None, estimator="mean-normalized-sgd", accumulate_multiple_batches=1, normalize_by_observations=True,
                      log_step_size=False, update_input_layer_weights=True, statistics_smoothing=None, trace_factor=None, initial_activations=None,
                      input_smoothing=None, input_trace_factor=0.5, input_initial_activations=None):
        """center: (Ws, biases) of the centred-L2 regulariser's centre, Ws[l] [out, in].  statistics_smoothing: per layer None /
        "no-statistics", "none" or "exponential-trace" (the output layer keeps none); trace_factor per layer; initial_activations: per
        layer None or (mean, standard deviation) of its output; the input_* arguments are the same for the last preprocessing layer.
        Resets the mini-batch counter and the activation statistics."""
        cfg = _lib.NnStepCfg()
        self.L.amx_nnstep_default_cfg(C.byref(cfg))
        n = self.n_layers
        cfg.learning_rate, cfg.bias_learning_rate = float(learning_rate), float(bias_learning_rate)

        def per_layer(v, dtype, what):
            if v is None:
                return None
            a = np.ascontiguousarray(v, dtype=dtype)
            if a.shape != (n,):
                raise ValueError("%s has shape %s, the network %d layers" % (what, a.shape, n))
            return a
        keep = [per_layer(layer_learning_rate, np.float32, "layer_learning_rate"), per_layer(regularization_constant, np.float32, "regularization_constant"),
                per_layer(trainable, np.int32, "trainable")]
        cfg.layer_learning_rate, cfg.regularization_constant, cfg.trainable = _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2])
        cfg.regularizer = regularizer if isinstance(regularizer, int) else self.REGULARIZERS[regularizer]
        cfg.estimator = estimator if isinstance(estimator, int) else self.ESTIMATORS[estimator]
        if center is not None:
            cw = [np.ascontiguousarray(w, dtype=np.float32) for w in center[0]]
            cb = [np.ascontiguousarray(b, dtype=np.float32) for b in center[1]]
            if len(cw) != n or len(cb) != n:
                raise ValueError("the centre has %d / %d layers, the network %d" % (len(cw), len(cb), n))
            if any(b.shape != (w.shape[0],) for w, b in zip(cw, cb)):
                raise ValueError("a centre bias does not match its weights")
            ind, outd = np.array([w.shape[1] for w in cw], np.int32), np.array([w.shape[0] for w in cw], np.int32)
            Wp, Bp = (C.c_void_p * n)(*[w.ctypes.data for w in cw]), (C.c_void_p * n)(*[b.ctypes.data for b in cb])
            keep += [cw, cb, ind, outd, Wp, Bp]
            cfg.center_W, cfg.center_bias = C.cast(Wp, C.c_void_p), C.cast(Bp, C.c_void_p)
            cfg.center_in_dim, cfg.center_out_dim = ind.ctypes.data, outd.ctypes.data
        self._smoothing = [self.SMOOTHING[m] for m in (statistics_smoothing or [None] * n)]
        if len(self._smoothing) != n:
            raise ValueError("statistics_smoothing has %d entries, the network %d layers" % (len(self._smoothing), n))
        keep.append(np.array(self._smoothing, np.int32))
        cfg.statistics_smoothing = keep[-1].ctypes.data
        keep.append(per_layer(trace_factor, np.float32, "trace_factor"))
        cfg.trace_factor = _ptr(keep[-1])
        if initial_activations is not None:
            means = [None if a is None else np.ascontiguousarray(a[0], dtype=np.float32) for a in initial_activations]
            devs = [None if a is None else np.ascontiguousarray(a[1], dtype=np.float32) for a in initial_activations]
            for l, m in enumerate(means):
                if m is not None and (m.shape != (self.layout.out_dim[l],) or devs[l].shape != m.shape):
                    raise ValueError("initial_activations[%d] does not match the layer's %d outputs" % (l, self.layout.out_dim[l]))
            Mp = (C.c_void_p * n)(*[None if m is None else m.ctypes.data for m in means])
            Dp = (C.c_void_p * n)(*[None if d is None else d.ctypes.data for d in devs])
            keep += [means, devs, Mp, Dp]
            cfg.initial_activation_mean, cfg.initial_activation_stddev = C.cast(Mp, C.c_void_p), C.cast(Dp, C.c_void_p)
        self._input_smoothing = self.SMOOTHING[input_smoothing]
        cfg.input_smoothing, cfg.input_trace_factor = self._input_smoothing, float(input_trace_factor)
        if input_initial_activations is not None:
            im, idv = (np.ascontiguousarray(a, dtype=np.float32) for a in input_initial_activations)
            if im.shape != (self.feature_dim,) or idv.shape != im.shape:
                raise ValueError("input_initial_activations does not match the %d features" % self.feature_dim)
            keep += [im, idv]
            cfg.input_initial_mean, cfg.input_initial_stddev = im.ctypes.data, idv.ctypes.data
        cfg.accumulate_multiple_batches = int(accumulate_multiple_batches)
        cfg.normalize_by_observations, cfg.log_step_size = int(bool(normalize_by_observations)), int(bool(log_step_size))
        cfg.update_input_layer_weights = int(bool(update_input_layer_weights))
        _lib.check(self.L.amx_nntrain_set_estimator(self.h, C.byref(cfg)))

    def _info(self, st):
        return {"minibatch": int(st.minibatch), "updated": bool(st.updated), "n_observations": int(st.n_observations),
                "n_classification_errors": int(st.n_classification_errors), "total_weight": float(st.total_weight), "objective": float(st.objective),
                "criterion_objective": float(st.criterion_objective), "step_size": np.array(st.step_size[:self.n_layers], np.float32)}

    def step_accumulate_dev(self, feats_dev, feats_stride, T, emission_dev, weight_dev=None):
        """one mini-batch into the group's statistics (arguments as accumulate_dev's, without the buffer)"""
        _lib.check(self.L.amx_nntrain_step_accumulate_dev(self.h, _ptr(feats_dev), int(feats_stride), int(T), _ptr(emission_dev), _ptr(weight_dev)))

    def step_estimate_dev(self):
        """finalize the group and run the estimator on it, whatever the mini-batch counter says"""
        _lib.check(self.L.amx_nntrain_step_estimate_dev(self.h))

    def step_dev(self, feats_dev, feats_stride, T, emission_dev, weight_dev=None, info=True):
        """step_accumulate_dev, then step_estimate_dev when the counter is a multiple of accumulate_multiple_batches; returns the
        group's info dict (one small device-to-host copy) unless info is False"""
        st = _lib.NnStepInfo()
        _lib.check(self.L.amx_nntrain_step_dev(self.h, _ptr(feats_dev), int(feats_stride), int(T), _ptr(emission_dev), _ptr(weight_dev),
                                               C.byref(st) if info else None))
        return self._info(st) if info else None

    def step_info(self):
        st = _lib.NnStepInfo()
        _lib.check(self.L.amx_nntrain_step_info(self.h, C.byref(st)))
        return self._info(st)

    def estimate(self, acc):
        """Nn::BatchEstimator on a flat accumulator (read(), combine_nn_statistics(), or an all-reduced device buffer)"""
        a, st = self._host(acc), _lib.NnStepInfo()
        _lib.check(self.L.amx_nntrain_estimate(self.h, a.ctypes.data, C.byref(st)))
        return self._info(st)

    def parameters(self, image=0):
        """[(W [out, in], bias [out])] per layer; image 0 = what the forward GEMM reads, 1 = the transposed image of the backward GEMM"""
        y, res = self.layout, []
        for l in range(self.n_layers):
            W, b = np.zeros((y.out_dim[l], y.in_dim[l]), np.float32), np.zeros(y.out_dim[l], np.float32)
            _lib.check(self.L.amx_nntrain_get_parameters(self.h, l, int(image), W.ctypes.data, b.ctypes.data))
            res.append((W, b))
        return res

    def step_statistics(self):
        """[(G [in, out], g [out])] per layer: the group's gradient, after a step the finalized gradient"""
        y, res = self.layout, []
        for l in range(self.n_layers):
            G, g = np.zeros((y.in_dim[l], y.out_dim[l]), np.float32), np.zeros(y.out_dim[l], np.float32)
            _lib.check(self.L.amx_nntrain_get_step_statistics(self.h, l, G.ctypes.data, g.ctypes.data))
            res.append((G, g))
        return res

    def activation_statistics(self):
        """{layer: (mean, variance)} of the layers that keep statistics (getActivationMean / getActivationVariance); layer -1 is the
        last preprocessing layer"""
        res = {}
        modes = [getattr(self, "_input_smoothing", 0)] + list(getattr(self, "_smoothing", []))[:-1]
        for p, mode in enumerate(modes):
            if mode == _lib.AMX_NNSTEP_STAT_NO_STATISTICS:
                continue
            n = self.layout.in_dim[p]
            mean, var = np.zeros(n, np.float32), np.zeros(n, np.float32)
            _lib.check(self.L.amx_nntrain_get_activation_statistics(self.h, p - 1, mean.ctypes.data, var.ctypes.data))
            res[p - 1] = (mean, var)
        return res

    def layer_input(self, layer, T):
        """the input of `layer` as the last pass left it, [T, in] (rows of frames that did not enter the batch included)"""
        X = np.zeros((int(T), self.layout.in_dim[layer]), np.float32)
        _lib.check(self.L.amx_nntrain_get_layer_input(self.h, int(layer), int(T), X.ctypes.data))
        return X

    def save(self, prefix):
        """every layer's parameter matrix [out x (1 + in)], column 0 the bias, as `parameters-new` writes it: <prefix>-layer-<l+1>.bin
        (read_nn_matrix / layer_from_parameters read it back); for a layer that keeps activation statistics also
        <prefix>-layer-<l+1>-activation-mean.xml and -activation-standard-deviation.xml (`new-activations-*-file`: the mean and the
        square root of the variance; layer 0 in the names is the last preprocessing layer); returns the parameter paths"""
        paths = []
        for l, (W, b) in enumerate(self.parameters()):
            paths.append("%s-layer-%d.bin" % (prefix, l + 1))
            write_nn_matrix("bin:" + paths[-1], np.concatenate([b[:, None], W], axis=1))
        if self.ctx is not None:
            for l, (mean, var) in self.activation_statistics().items():
                with np.errstate(invalid="ignore"):
                    dev = np.sqrt(var, dtype=np.float32)
                for what, v in (("mean", mean), ("standard-deviation", dev)):
                    path = "%s-layer-%d-activation-%s.xml" % (prefix, l + 1, what)
                    _lib.check(self.L.amx_nn_vector_write_f32(os.fsencode(path), len(v), v.ctypes.data))
        return paths


def combine_nn_statistics(trainer, paths):
    """Nn::Statistics<f32>::combine: the first file read, the others added in single precision in the order given -> flat accumulator"""
    names = [os.fsencode(p) for p in paths]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    a = np.zeros(trainer.accumulator_size(), np.float64)
    _lib.check(trainer.L.amx_nnstat_combine(trainer.h, arr, len(names), a.ctypes.data))
    return a


def prior_from_class_counts(trainer, acc, back_off_count=1):
    """Nn::Prior::setFromClassCounts: log prior per network output from the accumulator's class counts and the trainer's class weights"""
    a = trainer._host(acc)
    out = np.zeros(trainer.n_outputs, np.float32)
    _lib.check(trainer.L.amx_prior_from_class_counts(trainer.h, a.ctypes.data, float(back_off_count), out.ctypes.data))
    return out


def mean_and_deviation(trainer, acc):
    """MeanAndVarianceTrainer::writeMeanAndStandardDeviation: (mean, standard deviation), f32 [feature_dim], from the accumulator's sums"""
    a = trainer._host(acc)
    mean, dev = np.zeros(trainer.feature_dim, np.float32), np.zeros(trainer.feature_dim, np.float32)
    _lib.check(trainer.L.amx_nnstat_mean_and_deviation(trainer.h, a.ctypes.data, mean.ctypes.data, dev.ctypes.data))
    return mean, dev


_CMLLR_CRITERIA = {"naive": _lib.AMX_CMLLR_NAIVE, "mmi-prime": _lib.AMX_CMLLR_MMI_PRIME, "hlda": _lib.AMX_CMLLR_HLDA}


class AffineFeatureTransformEstimator:
    """Speech::AffineFeatureTransformEstimator over Mm::AffineFeatureTransformAccumulator (CMLLR): per key the flat f64 accumulator
    [beta | k: M x (F + 1) | mean: F + 1 | cov: upper triangle of order F + 1 | G: M x that triangle (non-pooled models only)], its corpus
    pass on the device, its files, combine, estimate and score.

    With a GmmFeatureScorer created on a context the estimator accumulates; for host-only use (files, combine, estimate, score) pass
    gmm=None and model_dim, and pooled_variance (f32 [model_dim]) when the model has one covariance."""

    def __init__(self, gmm, feature_dim, n_keys=1, model_dim=None, pooled_variance=None):
        self.L = _lib.lib()
        self.gmm, self.h = gmm, None
        self.shape = _lib.CmllrShape()
        self.pooled_variance = None
        if gmm is not None:
            h = C.c_void_p()
            _lib.check(self.L.amx_cmllr_create(gmm.h, int(feature_dim), int(n_keys), C.byref(h)))
            self.h = h
            _lib.check(self.L.amx_cmllr_describe(h, C.byref(self.shape), None))
            if self.shape.pooled:
                self.pooled_variance = np.zeros(self.shape.model_dim, np.float32)
                _lib.check(self.L.amx_cmllr_describe(h, None, self.pooled_variance.ctypes.data))
        else:
            if pooled_variance is not None:
                self.pooled_variance = np.ascontiguousarray(pooled_variance, dtype=np.float32)
                model_dim = len(self.pooled_variance) if model_dim is None else model_dim
            if model_dim is None:
                raise ValueError("AffineFeatureTransformEstimator: without a scorer, model_dim or pooled_variance says what the model's dimension is")
            self.shape = _lib.CmllrShape(int(feature_dim), int(model_dim), int(n_keys), 0 if pooled_variance is None else 1)
            if self.key_size() == 0:   # the shape is refused: let the library say why
                _lib.check(self.L.amx_cmllr_score(C.byref(self.shape), None, None, None, 0, None))
        self.feature_dim, self.model_dim, self.n_keys, self.pooled = self.shape.feature_dim, self.shape.model_dim, self.shape.n_keys, bool(self.shape.pooled)

    def close(self):
        if self.h:
            self.L.amx_cmllr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def key_size(self):
        """doubles of ONE key's part of the accumulator (0: the shape is refused)"""
        return int(self.L.amx_cmllr_key_size(C.byref(self.shape)))

    def accumulator_size(self):
        return self.key_size() * self.n_keys

    @staticmethod
    def kernel_shape():
        """(frames per LDS stage, triangle cells per workgroup, model components per workgroup) of the G kernel"""
        s, c, m = C.c_int(), C.c_int(), C.c_int()
        _lib.lib().amx_cmllr_kernel_shape(C.byref(s), C.byref(c), C.byref(m))
        return s.value, c.value, m.value

    def set_tile(self, tile_components):
        """A/B runs and tests: the G kernel with 16 (default) or 48 model components per workgroup; the same bits either way"""
        if self.h is None:
            raise RuntimeError("AffineFeatureTransformEstimator.set_tile: created without a scorer")
        _lib.check(self.L.amx_cmllr_set_tile(self.h, int(tile_components)))

    def accumulate_dev(self, feats_dev, feats_ld, frame_offsets, seg_key, emission_dev, best_density_dev, acc_dev, best_density_ld=0, weight_dev=None):
        """add the segments' frames to their keys: emission_dev int32 (-1 skips a frame), best_density_dev u32 (matrix with best_density_ld
        columns, or one per frame with 0), weight_dev f64 or None, acc_dev f64 [accumulator_size()]"""
        if self.h is None:
            raise RuntimeError("AffineFeatureTransformEstimator.accumulate_dev: created without a scorer")
        off = _offsets(frame_offsets, "AffineFeatureTransformEstimator.accumulate_dev")
        keys = np.ascontiguousarray(seg_key, dtype=np.int32)
        if len(keys) != len(off) - 1:
            raise ValueError("seg_key holds %d keys for %d segments" % (len(keys), len(off) - 1))
        _lib.check(self.L.amx_cmllr_accumulate_dev(self.h, _ptr(feats_dev), int(feats_ld), len(keys), off.ctypes.data, keys.ctypes.data, _ptr(emission_dev),
                                                   _ptr(best_density_dev), int(best_density_ld), _ptr(weight_dev), _ptr(acc_dev)))

    def _key(self, acc_host, key):
        a = np.ascontiguousarray(acc_host, dtype=np.float64).reshape(-1)
        n = self.key_size()
        if a.size == n and key in (0, None):
            return a
        if a.size != n * self.n_keys or key is None or not 0 <= key < self.n_keys:
            raise ValueError("accumulator has %d entries (%d per key, %d keys), key %r" % (a.size, n, self.n_keys, key))
        return a[key * n:(key + 1) * n]

    def members(self, acc_host, key=0):
        """dict(beta, k [M, F+1], mean [F+1], cov [F+1, F+1] upper triangle, G [M, F+1, F+1] upper triangles or None) of one key"""
        a, M, R = self._key(acc_host, key), self.model_dim, self.feature_dim + 1
        iu = np.triu_indices(R)
        tri = len(iu[0])
        out = dict(beta=a[0], k=a[1:1 + M * R].reshape(M, R).copy(), mean=a[1 + M * R:1 + M * R + R].copy(), G=None)
        p = 1 + M * R + R
        cov = np.zeros((R, R))
        cov[iu] = a[p:p + tri]
        out["cov"] = cov
        if not self.pooled:
            G = np.zeros((M, R, R))
            for i in range(M):
                G[i][iu] = a[p + tri * (i + 1):p + tri * (i + 2)]
            out["G"] = G
        return out

    def write(self, acc_host, path, key=0):
        """one key's accumulator as the reference's binary accumulator file (type tag first)"""
        a = self._key(acc_host, key)
        _lib.check(self.L.amx_cmllr_accumulator_write(C.byref(self.shape), _ptr(self.pooled_variance), a.ctypes.data, os.fsencode(path)))

    def read(self, path):
        """accumulator file -> one key's flat accumulator; the file must be of this estimator's shape"""
        n = self.key_size()
        a = np.zeros(max(n, 1), np.float64)
        _lib.check(self.L.amx_cmllr_accumulator_read(C.byref(self.shape), _ptr(self.pooled_variance), os.fsencode(path), a.ctypes.data))
        return a[:n]

    def combine(self, acc_host, other, other_acc, weight=1.0, key=0, other_key=0):
        """combine(other, weight): a copy of this key's accumulator plus weight times the other estimator's"""
        a = self._key(acc_host, key).copy()
        b = other._key(other_acc, other_key)
        _lib.check(self.L.amx_cmllr_combine(C.byref(self.shape), _ptr(self.pooled_variance), a.ctypes.data, C.byref(other.shape),
                                            _ptr(other.pooled_variance), b.ctypes.data, float(weight)))
        return a

    def estimate(self, acc_host, key=0, iterations=10, min_observation_weight=2000.0, criterion="mmi-prime", initial=None, details=False):
        """finalize + estimate: the transform f32 [M, F + 1]; details=True: (transform, dict(estimated, transform64, iterations))"""
        a, M, R = self._key(acc_host, key), self.model_dim, self.feature_dim + 1
        ini, cols = None, 0
        if initial is not None:
            ini = np.ascontiguousarray(initial, dtype=np.float32)
            if ini.ndim != 2 or ini.shape[0] != M:
                raise ValueError("the initial transform must have %d rows" % M)
            cols = ini.shape[1]
        out, out64 = np.zeros((M, R), np.float32), np.zeros((M, R), np.float64)
        its = np.zeros((max(int(iterations), 0), M, R), np.float64)
        est = C.c_int(0)
        _lib.check(self.L.amx_cmllr_estimate(C.byref(self.shape), _ptr(self.pooled_variance), a.ctypes.data, int(iterations), float(min_observation_weight),
                                             _CMLLR_CRITERIA[criterion], _ptr(ini), cols, out.ctypes.data, out64.ctypes.data,
                                             its.ctypes.data if its.size else None, C.byref(est)))
        return (out, dict(estimated=bool(est.value), transform64=out64, iterations=its)) if details else out

    def score(self, acc_host, transform, key=0, criterion="mmi-prime"):
        a = self._key(acc_host, key)
        t = np.ascontiguousarray(transform, dtype=np.float32)
        if t.shape != (self.model_dim, self.feature_dim + 1):
            raise ValueError("the transform must be [%d, %d]" % (self.model_dim, self.feature_dim + 1))
        s = C.c_double()
        _lib.check(self.L.amx_cmllr_score(C.byref(self.shape), _ptr(self.pooled_variance), a.ctypes.data, t.ctypes.data, _CMLLR_CRITERIA[criterion], C.byref(s)))
        return s.value


def write_transform(path, transform):
    """a transform f32 [rows, columns] as the XML matrix file the reference's estimator writes per key (`transform-directory`)"""
    t = np.ascontiguousarray(transform, dtype=np.float32)
    if t.ndim != 2:
        raise ValueError("write_transform: a matrix is wanted")
    _lib.check(_lib.lib().amx_cmllr_transform_write(os.fsencode(path), t.shape[0], t.shape[1], t.ctypes.data))


def read_transform(path):
    """XML matrix file (a key's transform, an `initial-transform`) -> f32 [rows, columns]"""
    L = _lib.lib()
    r, c, p = C.c_int(), C.c_int(), C.c_void_p()
    _lib.check(L.amx_cmllr_transform_read(os.fsencode(path), C.byref(r), C.byref(c), C.byref(p)))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(r.value, c.value)).copy()
    finally:
        L.amx_free(p)


class AffineFeatureTransform:
    """the application of CMLLR transforms: y = A_key [1, x] with the key chosen per segment inside one launch; a key without a
    transform passes its segments through (the first model_dim components)"""

    def __init__(self, ctx, model_dim, feature_dim, n_keys):
        self.ctx, self.L = ctx, ctx.L
        self.model_dim, self.feature_dim, self.n_keys = int(model_dim), int(feature_dim), int(n_keys)

    def apply_dev(self, transforms_dev, has_transform, frame_offsets, seg_key, in_dev, in_ld, out_dev, out_ld):
        """transforms_dev f32 [n_keys, model_dim, feature_dim + 1] on the device, has_transform [n_keys] on the host; returns the number of
        segments that got the identity"""
        off = _offsets(frame_offsets, "AffineFeatureTransform.apply_dev")
        keys = np.ascontiguousarray(seg_key, dtype=np.int32)
        has = np.ascontiguousarray(has_transform, dtype=np.int32)
        if len(keys) != len(off) - 1 or len(has) != self.n_keys:
            raise ValueError("seg_key holds %d keys for %d segments, has_transform %d flags for %d keys" % (len(keys), len(off) - 1, len(has), self.n_keys))
        n = C.c_int(0)
        _lib.check(self.L.amx_cmllr_apply_dev(self.ctx.h, _ptr(transforms_dev), has.ctypes.data, self.n_keys, self.model_dim, self.feature_dim, _ptr(in_dev),
                                              int(in_ld), len(keys), off.ctypes.data, keys.ctypes.data, _ptr(out_dev), int(out_ld), C.byref(n)))
        return n.value


_MLLR_MODES = {"full": _lib.AMX_MLLR_FULL, "shift": _lib.AMX_MLLR_SHIFT, "band": _lib.AMX_MLLR_BAND, "semi-tied": _lib.AMX_MLLR_SEMI_TIED}


class ModelTransformEstimator:
    """Speech::ModelTransformEstimator over Mm::FullAdaptorViterbiEstimator / Mm::ShiftAdaptorViterbiEstimator (MLLR): per (key, leaf) the
    flat f64 accumulator ([count_Z | Z: D x (D + 1) | count_G | G: (D + 1) x (D + 1)], shift: [count | beta: D | shift: D]), its corpus
    pass on the device, its files and adaptor().

    leaf_of_mixture is the reference's leafIndex_ as MllrAdaptation.cc indexes it, with the mixture index.  With a GmmFeatureScorer
    created on a context the estimator accumulates; for host-only use (files, estimate) pass gmm=None and dim."""

    def __init__(self, gmm, mode, n_leafs, leaf_of_mixture, n_keys=1, dim=None):
        self.L = _lib.lib()
        self.gmm, self.h = gmm, None
        if mode not in _MLLR_MODES:
            raise ValueError("ModelTransformEstimator: unknown mode %r" % (mode,))
        self.leaf_of_mixture = np.ascontiguousarray(leaf_of_mixture, dtype=np.int32)
        self.shape = _lib.MllrShape()
        if gmm is not None:
            h = C.c_void_p()
            _lib.check(self.L.amx_mllr_create(gmm.h, _MLLR_MODES[mode], int(n_keys), int(n_leafs), self.leaf_of_mixture.ctypes.data, C.byref(h)))
            self.h = h
            _lib.check(self.L.amx_mllr_describe(h, C.byref(self.shape)))
        else:
            if dim is None:
                raise ValueError("ModelTransformEstimator: without a scorer, dim says what the model's dimension is")
            self.shape = _lib.MllrShape(_MLLR_MODES[mode], int(dim), int(n_leafs), int(n_keys))
            if self.key_size() == 0:   # the shape is refused: let the library say why
                _lib.check(self.L.amx_mllr_accumulator_read(C.byref(self.shape), None, None, None, None))
        self.mode, self.dim, self.n_leafs, self.n_keys = mode, self.shape.dim, self.shape.n_leafs, self.shape.n_keys
        self.n_mixtures = len(self.leaf_of_mixture)

    def close(self):
        if self.h:
            self.L.amx_mllr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def leaf_size(self):
        return int(self.L.amx_mllr_leaf_size(C.byref(self.shape)))

    def key_size(self):
        """doubles of ONE key's part of the accumulator (0: the shape is refused)"""
        return int(self.L.amx_mllr_key_size(C.byref(self.shape)))

    def accumulator_size(self):
        return self.key_size() * self.n_keys

    @staticmethod
    def kernel_shape():
        """(frames per LDS stage, cells per workgroup) of the accumulation kernel"""
        s, c = C.c_int(), C.c_int()
        _lib.lib().amx_mllr_kernel_shape(C.byref(s), C.byref(c))
        return s.value, c.value

    def accumulate_dev(self, feats_dev, feats_ld, frame_offsets, seg_key, emission_dev, best_density_dev, acc_dev, best_density_ld=0, weight_dev=None):
        """add the segments' frames to (their key, their emission's leaf): arguments as AffineFeatureTransformEstimator.accumulate_dev"""
        if self.h is None:
            raise RuntimeError("ModelTransformEstimator.accumulate_dev: created without a scorer")
        off = _offsets(frame_offsets, "ModelTransformEstimator.accumulate_dev")
        keys = np.ascontiguousarray(seg_key, dtype=np.int32)
        if len(keys) != len(off) - 1:
            raise ValueError("seg_key holds %d keys for %d segments" % (len(keys), len(off) - 1))
        _lib.check(self.L.amx_mllr_accumulate_dev(self.h, _ptr(feats_dev), int(feats_ld), len(keys), off.ctypes.data, keys.ctypes.data, _ptr(emission_dev),
                                                  _ptr(best_density_dev), int(best_density_ld), _ptr(weight_dev), _ptr(acc_dev)))

    def _key(self, acc_host, key):
        a = np.ascontiguousarray(acc_host, dtype=np.float64).reshape(-1)
        n = self.key_size()
        if a.size == n and key in (0, None):
            return a
        if a.size != n * self.n_keys or key is None or not 0 <= key < self.n_keys:
            raise ValueError("accumulator has %d entries (%d per key, %d keys), key %r" % (a.size, n, self.n_keys, key))
        return a[key * n:(key + 1) * n]

    def write(self, acc_host, path, key=0, cluster_id="", min_observation=1000.0, min_silence_observation=500.0, node_count=None, map_ids=()):
        """one key's accumulator as the reference's binary accumulator file (type tag first); map_ids: the tree's node ids"""
        a = self._key(acc_host, key)
        cnt = None if node_count is None else np.ascontiguousarray(node_count, dtype=np.float64)
        ids = np.ascontiguousarray(map_ids, dtype=np.int32)
        _lib.check(self.L.amx_mllr_accumulator_write(C.byref(self.shape), a.ctypes.data, os.fsencode(cluster_id), float(min_observation),
                                                     float(min_silence_observation), 0 if cnt is None else len(cnt), _ptr(cnt), len(ids),
                                                     ids.ctypes.data if len(ids) else None, os.fsencode(path)))

    def read(self, path, thresholds=False):
        """accumulator file -> one key's flat accumulator (thresholds=True: and the file's two thresholds)"""
        n = self.key_size()
        a = np.zeros(max(n, 1), np.float64)
        mo, ms = C.c_double(), C.c_double()
        _lib.check(self.L.amx_mllr_accumulator_read(C.byref(self.shape), os.fsencode(path), a.ctypes.data, C.byref(mo), C.byref(ms)))
        return (a[:n], mo.value, ms.value) if thresholds else a[:n]

    def estimate(self, acc_host, tree, key=0, min_observation=1000.0, min_silence_observation=500.0, rcond=0.0):
        """adaptor() of one key.  tree: dict(root, left, right, previous, leaf_number [n_ids] with -1 for none, leaf_list (node ids in
        leafList() order), silence_mixtures (ascending)).  Returns dict(matrix_ids, matrices [n, D, D + 1] (shift: [n, D]),
        matrix_of_mixture, node_count, root_fallback, silence_fallback)"""
        a, D = self._key(acc_host, key), self.dim
        arr = {k: np.ascontiguousarray(tree[k], dtype=np.int32) for k in ("left", "right", "previous", "leaf_number", "leaf_list", "silence_mixtures")}
        n_ids = len(arr["left"])
        if not (len(arr["right"]) == len(arr["previous"]) == len(arr["leaf_number"]) == n_ids):
            raise ValueError("ModelTransformEstimator.estimate: left, right, previous and leaf_number must have one entry per node id")
        t = _lib.MllrTree(n_ids, int(tree["root"]), arr["left"].ctypes.data, arr["right"].ctypes.data, arr["previous"].ctypes.data,
                          arr["leaf_number"].ctypes.data, len(arr["leaf_list"]), arr["leaf_list"].ctypes.data, len(arr["silence_mixtures"]),
                          arr["silence_mixtures"].ctypes.data)
        cap = len(arr["leaf_list"]) + len(arr["silence_mixtures"]) + 1
        per = (D,) if self.mode == "shift" else (D, D + 1)
        ids, mats = np.zeros(cap, np.int32), np.zeros((cap,) + per, np.float64)
        index, cnt = np.zeros(self.n_mixtures, np.int32), np.zeros(max(n_ids, 1), np.float64)
        n, fl = C.c_int(0), C.c_int(0)
        _lib.check(self.L.amx_mllr_estimate(C.byref(self.shape), a.ctypes.data, C.byref(t), self.n_mixtures, self.leaf_of_mixture.ctypes.data,
                                            float(min_observation), float(min_silence_observation), float(rcond), C.byref(n), ids.ctypes.data,
                                            mats.ctypes.data, index.ctypes.data, cnt.ctypes.data, C.byref(fl)))
        return dict(matrix_ids=ids[:n.value].copy(), matrices=mats[:n.value].copy(), matrix_of_mixture=index, node_count=cnt[:n_ids],
                    root_fallback=bool(fl.value & _lib.AMX_MLLR_ROOT_FALLBACK), silence_fallback=bool(fl.value & _lib.AMX_MLLR_SILENCE_FALLBACK))

    def write_adaptor(self, path, matrix_ids, matrices, matrix_of_mixture, cluster_id=""):
        """FullAdaptor::write / ShiftAdaptor::write behind the type tag"""
        ids = np.ascontiguousarray(matrix_ids, dtype=np.int32)
        mats = np.ascontiguousarray(matrices, dtype=np.float64)
        index = np.ascontiguousarray(matrix_of_mixture, dtype=np.int32)
        if mats.shape != (len(ids),) + ((self.dim,) if self.mode == "shift" else (self.dim, self.dim + 1)):
            raise ValueError("write_adaptor: matrices of shape %r for %d ids" % (mats.shape, len(ids)))
        _lib.check(self.L.amx_mllr_adaptor_write(C.byref(self.shape), os.fsencode(cluster_id), len(ids), ids.ctypes.data, mats.ctypes.data, len(index),
                                                 index.ctypes.data, os.fsencode(path)))

    def read_adaptor(self, path, max_matrices=65535):
        per = (self.dim,) if self.mode == "shift" else (self.dim, self.dim + 1)
        ids, mats = np.zeros(max_matrices, np.int32), np.zeros((max_matrices,) + per, np.float64)
        index, n = np.zeros(self.n_mixtures, np.int32), C.c_int(0)
        _lib.check(self.L.amx_mllr_adaptor_read(C.byref(self.shape), os.fsencode(path), int(max_matrices), C.byref(n), ids.ctypes.data, mats.ctypes.data,
                                                self.n_mixtures, index.ctypes.data))
        return dict(matrix_ids=ids[:n.value].copy(), matrices=mats[:n.value].copy(), matrix_of_mixture=index)


class MixtureSetAdaptor:
    """Am::MixtureSetAdaptor's mean adaptation for one key: FullAdaptor / ShiftAdaptor::adaptMixtureSet on the device.  The adapted mean
    table [n_means, D] f32 goes to a device buffer; the caller copies it out and creates the adapted scorer from it."""

    def __init__(self, estimator):
        if estimator.h is None:
            raise RuntimeError("MixtureSetAdaptor: the estimator was created without a scorer")
        self.est, self.L = estimator, estimator.L

    def adapt_means_dev(self, matrix_ids, matrices, matrix_of_mixture, out_dev):
        ids = np.ascontiguousarray(matrix_ids, dtype=np.int32)
        mats = np.ascontiguousarray(matrices, dtype=np.float64)
        index = np.ascontiguousarray(matrix_of_mixture, dtype=np.int32)
        e = self.est
        if mats.shape != (len(ids),) + ((e.dim,) if e.mode == "shift" else (e.dim, e.dim + 1)) or len(index) != e.n_mixtures:
            raise ValueError("adapt_means_dev: matrices of shape %r for %d ids, %d indices for %d mixtures" % (mats.shape, len(ids), len(index), e.n_mixtures))
        _lib.check(self.L.amx_mllr_adapt_means_dev(e.h, len(ids), ids.ctypes.data, mats.ctypes.data, index.ctypes.data, _ptr(out_dev)))


class EbwAccumulator:
    """The corpus pass of Speech::SegmentwiseGmmTrainer into Mm::EbwDiscriminativeMixtureSetEstimator's accumulators: lattice arc weights
    (what Fsa::posteriorE left on the arcs) become numerator and denominator statistics in ONE flat f64 buffer,
    [numerator: amx_gmm_accumulate_dev's layout][denominator slot weights | mean weights | mean sums |
    covariance weights | covariance sums][objective].

    weight_threshold and viterbi are the reference's parameters with its defaults; viterbi=False is refused."""

    VIEWS = ("num_mixture_weights", "num_mean_weights", "num_mean_sums", "num_cov_weights", "num_cov_sums", "den_density_weights",
             "den_mean_weights", "den_mean_sums", "den_cov_weights", "den_cov_sums", "objective")

    def __init__(self, gmm, weight_threshold=None, viterbi=True):
        self.L = _lib.lib()
        self.gmm, self.h = gmm, None
        cfg = _lib.EbwCfg()
        self.L.amx_ebw_cfg_default(C.byref(cfg))
        if weight_threshold is not None:
            cfg.weight_threshold = float(weight_threshold)
        cfg.viterbi = 1 if viterbi else 0
        h = C.c_void_p()
        _lib.check(self.L.amx_ebw_create(gmm.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.weight_threshold = cfg.weight_threshold
        self.layout = _lib.EbwOffsets()
        _lib.check(self.L.amx_ebw_layout(h, C.byref(self.layout)))

    def close(self):
        if self.h:
            self.L.amx_ebw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulator_size(self):
        return int(self.L.amx_ebw_accumulator_size(self.h))

    def view(self, acc, name):
        """the named part of a flat accumulator (numpy array or tensor): a view, shaped [n] or [n, dim]"""
        o = self.layout
        n = {"num_mixture_weights": o.n_slots, "den_density_weights": o.n_slots, "num_mean_weights": o.n_means, "den_mean_weights": o.n_means,
             "num_cov_weights": o.n_covariances, "den_cov_weights": o.n_covariances, "objective": 1}
        if name not in self.VIEWS:
            raise KeyError("EbwAccumulator.view: no part called %r" % (name,))
        b = getattr(o, name)
        if name in n:
            return acc[b:b + n[name]]
        rows = o.n_means if "mean" in name else o.n_covariances
        return acc[b:b + rows * o.dim].reshape(rows, o.dim)

    def accumulate_dev(self, feats_dev, feats_ld, frame_offsets, arc_offsets, arc_weight, item_offsets, item_frame, item_emission, acc_dev):
        """add a batch of segments: segment s owns the feature rows [frame_offsets[s], frame_offsets[s + 1]) and the arcs
        [arc_offsets[s], arc_offsets[s + 1]); arc a carries arc_weight[a] (f32, signed) and the items [item_offsets[a], item_offsets[a + 1]),
        each a frame relative to the segment and an emission index.  The tables are host arrays."""
        off = _offsets(frame_offsets, "EbwAccumulator.accumulate_dev")
        arcs = np.ascontiguousarray(arc_offsets, dtype=np.int64)
        items = np.ascontiguousarray(item_offsets, dtype=np.int64)
        w = np.ascontiguousarray(arc_weight, dtype=np.float32)
        fr = np.ascontiguousarray(item_frame, dtype=np.int32)
        em = np.ascontiguousarray(item_emission, dtype=np.int32)
        if len(arcs) != len(off) or len(items) != len(w) + 1 or (len(arcs) and arcs[-1] != len(w)) or len(fr) != len(em) or items[-1] != len(fr):
            raise ValueError("EbwAccumulator.accumulate_dev: %d segments, %d arc offsets, %d arcs, %d item offsets, %d / %d items"
                             % (len(off) - 1, len(arcs), len(w), len(items), len(fr), len(em)))
        _lib.check(self.L.amx_ebw_accumulate_dev(self.h, _ptr(feats_dev), int(feats_ld), len(off) - 1, off.ctypes.data, arcs.ctypes.data,
                                                 w.ctypes.data, items.ctypes.data, fr.ctypes.data, em.ctypes.data, _ptr(acc_dev)))

    def accumulate_objective(self, objective, acc_dev):
        """accumulateObjectiveFunction: one segment's objective (f32, widened) into the buffer's last cell"""
        _lib.check(self.L.amx_ebw_accumulate_objective(self.h, float(np.float32(objective)), _ptr(acc_dev)))

    @staticmethod
    def kernel_shape():
        """(elements per workgroup of the sort and the scan, keys a chain stages at a time, threads per workgroup)"""
        b, s, t = C.c_int(), C.c_int(), C.c_int()
        _lib.lib().amx_ebw_kernel_shape(C.byref(b), C.byref(s), C.byref(t))
        return b.value, s.value, t.value

    def last_shape(self):
        """what the last accumulate_dev ran: dict(item_sort_passes, list_sort_passes, item_blocks, list_blocks, item_table_recursed,
        list_table_recursed), all 0 for a call that ended before the sort"""
        s = _lib.EbwCallShape()
        _lib.check(self.L.amx_ebw_last_shape(self.h, C.byref(s)))
        return {n: (bool(getattr(s, n)) if n.endswith("recursed") else int(getattr(s, n))) for n, _ in s._fields_}

    def last_keys(self):
        """the keys of the last accumulate_dev in ascending (frame, mixture, side): dict(frame, mixture, side, weight, slot)"""
        n = C.c_int(0)
        _lib.check(self.L.amx_ebw_last_keys(self.h, 0, C.byref(n), None, None, None, None, None))
        k = max(n.value, 1)
        frame, mix, side = np.zeros(k, np.int64), np.zeros(k, np.int32), np.zeros(k, np.int32)
        weight, slot = np.zeros(k, np.float64), np.zeros(k, np.int32)
        _lib.check(self.L.amx_ebw_last_keys(self.h, k, C.byref(n), frame.ctypes.data, mix.ctypes.data, side.ctypes.data, weight.ctypes.data,
                                            slot.ctypes.data))
        return dict(frame=frame[:n.value], mixture=mix[:n.value], side=side[:n.value], weight=weight[:n.value], slot=slot[:n.value])

    # ---- host side: the reference's binary estimator file and the file-level sum; `model` is the model dict of the statistics

    @staticmethod
    def topology_size(model):
        """doubles of the flat accumulator, from the model's topology alone"""
        keep = []
        return int(_lib.lib().amx_ebw_topology_accumulator_size(C.byref(_gmm_struct(model, 1.0, 1.0, keep))))

    @staticmethod
    def _host(model, acc, who):
        a = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1)
        n = EbwAccumulator.topology_size(model)   # 0: the topology is refused, and the library says why
        if n and a.size != n:
            raise ValueError("%s: accumulator has %d entries, the model's has %d" % (who, a.size, n))
        return a

    @staticmethod
    def write(model, acc_host, path):
        """Mm::EbwDiscriminativeMixtureSetEstimator's binary estimator file (magic "DTACC", version 2, denominator accumulators, objective)"""
        keep = []
        a = EbwAccumulator._host(model, acc_host, "EbwAccumulator.write")
        _lib.check(_lib.lib().amx_ebw_accumulator_write(C.byref(_gmm_struct(model, 1.0, 1.0, keep)), a.ctypes.data, os.fsencode(path)))

    @staticmethod
    def read(model, path):
        """estimator file -> flat accumulator; the file's topology must be the model's"""
        keep = []
        a = np.zeros(EbwAccumulator.topology_size(model), np.float64)
        _lib.check(_lib.lib().amx_ebw_accumulator_read(C.byref(_gmm_struct(model, 1.0, 1.0, keep)), os.fsencode(path), a.ctypes.data if a.size else None))
        return a

    @staticmethod
    def combine(model, acc_host, add_host):
        """combine-mixture-set-estimators for two accumulators: acc_host += add_host (in place when acc_host is a contiguous f64 array)"""
        keep = []
        a = EbwAccumulator._host(model, acc_host, "EbwAccumulator.combine")
        b = EbwAccumulator._host(model, add_host, "EbwAccumulator.combine")
        _lib.check(_lib.lib().amx_ebw_accumulator_combine(C.byref(_gmm_struct(model, 1.0, 1.0, keep)), a.ctypes.data, b.ctypes.data))
        return a


class EbwEstimator:
    """Mm::EbwDiscriminativeMixtureSetEstimator::estimate (with an i-smoothing set: ...WithISmoothing): the EBW update from the flat
    accumulator of EbwAccumulator.  Keyword arguments are the reference's parameters with its defaults: minimum_observation_weight (5),
    minimum_relative_weight (0), minimum_variance (0), normalize_mixture_weights (True), type ("global-rwth" | "local-rwth";
    "cambridge" is refused), step_size (1.1), minimum_icd (1), beta (1), sigma_minimum (None: sigma_minimum_factor times the smallest
    previous variance), sigma_minimum_factor (1e-5), number_of_iterations (100), i_smoothing_means (0), i_smoothing_weights (0),
    viterbi (True), estimator ("ebw"; "rprop" is refused), contract ("off" | "fma")."""

    TYPES = {"global-rwth": _lib.AMX_EBW_IC_GLOBAL_RWTH, "local-rwth": _lib.AMX_EBW_IC_LOCAL_RWTH, "cambridge": _lib.AMX_EBW_IC_CAMBRIDGE}
    NAMES = {"minimum_observation_weight": "min_observation_weight", "minimum_relative_weight": "min_relative_weight", "minimum_variance": "min_variance"}

    def __init__(self, **kw):
        self.L = _lib.lib()
        self.cfg = _lib.EbwEstimateCfg()
        self.L.amx_ebw_estimate_cfg_default(C.byref(self.cfg))
        for k, v in kw.items():
            k = self.NAMES.get(k, k)
            if k == "type":
                if v not in self.TYPES:
                    raise ValueError("EbwEstimator: unknown type of iteration constants %r" % (v,))
                self.cfg.iteration_constants = self.TYPES[v]
            elif k == "estimator":
                self.cfg.estimator = {"ebw": _lib.AMX_EBW_ESTIMATOR_EBW, "rprop": _lib.AMX_EBW_ESTIMATOR_RPROP}[v]
            elif k == "contract":
                self.cfg.contract = Context.CONTRACTS[v] if isinstance(v, str) else int(v)
            elif k == "sigma_minimum":
                self.cfg.sigma_minimum = -1.0 if v is None else float(v)
            elif hasattr(self.cfg, k):
                setattr(self.cfg, k, int(v) if k in ("normalize_mixture_weights", "number_of_iterations", "viterbi") else float(v))
            else:
                raise TypeError("EbwEstimator: unknown option %r" % (k,))

    def estimate(self, model, acc_host, previous, ismoothing=None):
        """model: the model dict the statistics were accumulated with; previous / ismoothing: model dicts on the same topology.
        Returns (new model dict, dict(i_smoothing_objective, sigma_minimum, n_removed, n_clamped, n_mean_fallback, n_floored,
        iteration_constants [new means]))"""
        keep = []
        a = EbwAccumulator._host(model, acc_host, "EbwEstimator.estimate")
        st = _gmm_struct(model, 1.0, 1.0, keep)
        ps = _gmm_struct(previous, 1.0, 1.0, keep)
        ist = _gmm_struct(ismoothing, 1.0, 1.0, keep) if ismoothing is not None else None
        info, icd, h = _lib.EbwEstimateInfo(), np.zeros(max(st.n_mean, 1), np.float64), C.c_void_p()
        _lib.check(self.L.amx_ebw_estimate(C.byref(st), a.ctypes.data, C.byref(ps), C.byref(ist) if ist is not None else None, C.byref(self.cfg),
                                           C.byref(h), C.byref(info), icd.ctypes.data))
        new = _mixture_set_to_dict(h)
        return new, dict(i_smoothing_objective=info.i_smoothing_objective, sigma_minimum=info.sigma_minimum, n_removed=info.n_removed,
                         n_clamped=info.n_clamped, n_mean_fallback=info.n_mean_fallback, n_floored=info.n_floored,
                         iteration_constants=icd[:new["means"].shape[0]].copy())


class LatticePosterior:
    """Arc posteriors of word lattices, a batch per call, left on the device: Fsa::posterior64 (mode "log"), posterior64 followed by
    Fsa::expm ("prob") and Fsa::posteriorE over an accuracy lattice ("expectation"), in f64 in the log semiring, every sum in the
    reference's order.  A lattice is a dict of host arrays: arc_offsets [n + 1] (state s owns the arcs [arc_offsets[s], arc_offsets[s + 1])
    in the automaton's own order), arc_target (state ids of this lattice), arc_weight, initial, final_flag [n], final_weight [n] and, for
    "expectation", arc_risk and final_risk.  The contract (the one fused multiply-add of the expectation pass) is the context's."""

    MODES = {"log": _lib.AMX_LATPOST_LOG, "prob": _lib.AMX_LATPOST_PROB, "expectation": _lib.AMX_LATPOST_EXPECTATION}
    INFO = tuple(n for n, _ in _lib.LatpostInfo._fields_)

    def __init__(self, ctx, mode="log", normalize=True, v_normalized=True, tolerance=100, potentials="auto"):
        self.L = _lib.lib()
        self.ctx, self.h = ctx, None
        if mode not in self.MODES:
            raise ValueError("LatticePosterior: unknown mode %r" % (mode,))
        if potentials not in ("auto", "global"):
            raise ValueError("LatticePosterior: potentials must be 'auto' or 'global', not %r" % (potentials,))
        cfg = _lib.LatpostCfg()
        self.L.amx_latpost_cfg_default(C.byref(cfg))
        cfg.mode, cfg.normalize, cfg.v_normalized, cfg.tolerance = self.MODES[mode], int(bool(normalize)), int(bool(v_normalized)), int(tolerance)
        cfg.potentials = _lib.AMX_LATPOST_POTENTIALS_GLOBAL if potentials == "global" else _lib.AMX_LATPOST_POTENTIALS_AUTO
        h = C.c_void_p()
        _lib.check(self.L.amx_latpost_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(h)))
        self.h, self.mode = h, mode

    def close(self):
        if self.h:
            self.L.amx_latpost_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def kernel_shape():
        """dict(threads, lds_states, wave_arcs): the potentials kernel's workgroup, the largest segment (states + 1) kept in LDS, the
        number of arcs from which a wave shares a state"""
        t, s, w = C.c_int(), C.c_int(), C.c_int()
        _lib.lib().amx_latpost_kernel_shape(C.byref(t), C.byref(s), C.byref(w))
        return dict(threads=t.value, lds_states=s.value, wave_arcs=w.value)

    def tables(self, lattices):
        """the call's CSR tables from a list of lattice dicts"""
        who, e = "LatticePosterior", self.mode == "expectation"
        so, ao, tgt, w, r, ini, ff, fw, fr = [0], [np.zeros(1, np.int64)], [], [], [], [], [], [], []
        n_arcs = 0
        for k, lat in enumerate(lattices):
            off = np.ascontiguousarray(lat["arc_offsets"], dtype=np.int64)
            n = len(off) - 1
            t = np.ascontiguousarray(lat["arc_target"], dtype=np.int32)
            if n < 0 or (n >= 0 and (off[0] != 0 or off[-1] != len(t))) or len(lat["arc_weight"]) != len(t) or len(lat["final_flag"]) != n or \
                    len(lat["final_weight"]) != n:
                raise ValueError("%s: lattice %d: %d states, %d arc offsets ending at %s, %d targets, %d weights" %
                                 (who, k, n, len(off), off[-1] if len(off) else None, len(t), len(lat["arc_weight"])))
            if e and ("arc_risk" not in lat or "final_risk" not in lat or len(lat["arc_risk"]) != len(t) or len(lat["final_risk"]) != n):
                raise ValueError("%s: lattice %d: mode 'expectation' needs arc_risk and final_risk" % (who, k))
            so.append(so[-1] + n)
            ao.append(off[1:] + n_arcs)
            n_arcs += len(t)
            tgt.append(t), w.append(np.asarray(lat["arc_weight"], np.float32)), ini.append(int(lat["initial"]))
            ff.append(np.asarray(lat["final_flag"]).astype(np.uint8)), fw.append(np.asarray(lat["final_weight"], np.float32))
            if e:
                r.append(np.asarray(lat["arc_risk"], np.float32)), fr.append(np.asarray(lat["final_risk"], np.float32))
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, dt), dtype=dt)   # noqa: E731
        return dict(n_seg=len(lattices), state_offsets=np.array(so, np.int64), arc_offsets=cat(ao, np.int64), arc_target=cat(tgt, np.int32),
                    arc_weight=cat(w, np.float32), arc_risk=cat(r, np.float32) if e else None, initial=np.array(ini, np.int32),
                    final_flag=cat(ff, np.uint8), final_weight=cat(fw, np.float32), final_risk=cat(fr, np.float32) if e else None)

    @classmethod
    def _info(cls, infos):
        return [{n: getattr(i, n) for n in cls.INFO} for i in infos]

    def run(self, lattices):
        """-> (arc weights, final weights, info): two f32 device tensors, one value per arc in the order of the input (lattice after
        lattice) and one per state, and a list of dicts per lattice (total_inv, total_inv_f32, expectation, forward_flow, backward_flow,
        flows_agree, vanishing_flow, reason, the counts).  A refused input raises AmxError and leaves nothing behind."""
        import torch
        t = self.tables(lattices)
        n_states, n_arcs = int(t["state_offsets"][-1]), len(t["arc_target"])
        dev = torch.device("cuda", self.ctx.device)
        arc_out, final_out = torch.empty(max(n_arcs, 1), dtype=torch.float32, device=dev), torch.empty(max(n_states, 1), dtype=torch.float32, device=dev)
        info = self.run_dev(t, arc_out, final_out)
        return arc_out[:n_arcs], final_out[:n_states], info

    def run_dev(self, t, arc_out_dev, final_out_dev):
        """the same into buffers of the caller's (t: what tables() returns)"""
        infos = (_lib.LatpostInfo * max(t["n_seg"], 1))()
        _lib.check(self.L.amx_latpost_run_dev(self.h, t["n_seg"], _ptr(t["state_offsets"]), _ptr(t["arc_offsets"]), _ptr(t["arc_target"]), _ptr(t["arc_weight"]),
                                              _ptr(t["arc_risk"]), _ptr(t["initial"]), _ptr(t["final_flag"]), _ptr(t["final_weight"]), _ptr(t["final_risk"]),
                                              _ptr(arc_out_dev), _ptr(final_out_dev), C.cast(infos, C.c_void_p)))
        return self._info(infos[:t["n_seg"]])

    def plan(self, lattices):
        """the host plan alone (no device): dict(discover_index, level_backward, level_forward, level_super, in_offsets, in_arc, final_order,
        info) over the call's states and arcs"""
        t = self.tables(lattices)
        n_states, n_arcs, n_seg = int(t["state_offsets"][-1]), len(t["arc_target"]), t["n_seg"]
        out = dict(discover_index=np.zeros(n_states, np.int32), level_backward=np.zeros(n_states, np.int32), level_forward=np.zeros(n_states, np.int32),
                   level_super=np.zeros(n_seg, np.int32), in_offsets=np.zeros(n_states + 1, np.int64), in_arc=np.full(n_arcs, -1, np.int32),
                   final_order=np.zeros(n_states, np.int32))
        infos = (_lib.LatpostInfo * max(n_seg, 1))()
        _lib.check(self.L.amx_latpost_plan_host(self.h, n_seg, _ptr(t["state_offsets"]), _ptr(t["arc_offsets"]), _ptr(t["arc_target"]), _ptr(t["arc_weight"]),
                                                _ptr(t["arc_risk"]), _ptr(t["initial"]), _ptr(t["final_flag"]), _ptr(t["final_weight"]), _ptr(t["final_risk"]),
                                                *(_ptr(out[k]) for k in ("discover_index", "level_backward", "level_forward", "level_super", "in_offsets",
                                                                         "in_arc", "final_order")), C.cast(infos, C.c_void_p)))
        out["info"] = self._info(infos[:n_seg])
        out["tables"] = t
        return out

    def last_timing(self):
        """DIAGNOSTIC: (plan ms, upload ms) of the last run: host wall time of the plan and of packing and uploading the tables"""
        a, b = C.c_double(), C.c_double()
        _lib.check(self.L.amx_latpost_last_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_potentials(self, n_states):
        """DIAGNOSTIC: dict(forward, backward, generalized_forward, generalized_backward) of the last run, per state over the call"""
        out = {k: np.zeros(n_states, np.float64) for k in ("forward", "backward", "generalized_forward", "generalized_backward")}
        _lib.check(self.L.amx_latpost_last_potentials(self.h, n_states, *(_ptr(out[k]) for k in ("forward", "backward", "generalized_forward",
                                                                                                 "generalized_backward"))))
        return out


class SegmentwiseNnTrainer:
    """Nn::SegmentwiseNnTrainer in full-batch mode (criteria MMI and ME) on a FeedForwardTrainer whose statistics are "base" and,
    for anything but the base statistics, "gradient": forward pass of a batch of segments, arc scores from the network's output, and the
    error signal collected from the arcs' posteriors, with frame rejection and cross-entropy smoothing, into the trainer's flat f64
    accumulator (include/amx.h, "NN sequence-discriminative training").  The model carries the log prior removed from the top bias
    already.  Numerator extraction, the best path (emission), the language-model part of the arc scores, the lattice forward-backward
    (LatticePosterior), `skip` and `objective` stay with the caller.  Arc tables: dict(arc_offsets [n_seg + 1], item_offsets
    [n_arcs + 1], item_frame, item_emission) of host arrays, the layout EbwAccumulator takes; item_frame counts from its segment's start."""

    ROLES = {"add": _lib.AMX_NNSEQ_ADD, "reject": _lib.AMX_NNSEQ_ADD_REJECT, "reject-clear": _lib.AMX_NNSEQ_ADD_REJECT_CLEAR}
    REASONS = {_lib.AMX_NNSEQ_SEG_OK: "ok", _lib.AMX_NNSEQ_SEG_SKIPPED: "skipped", _lib.AMX_NNSEQ_SEG_NO_ALIGNMENT: "no-alignment"}

    def __init__(self, trainer, weight_threshold=None, ce_smoothing_weight=0.0, frame_rejection_threshold=0.0, log_prior=None, prior_scale=0.0,
                 full_batch=True, accumulate_prior=False, label_type="emission-ids", keep_lattice_error=False):
        self.L, self.trainer, self.ctx, self.h = _lib.lib(), trainer, trainer.ctx, None
        cfg = _lib.NnSeqCfg()
        self.L.amx_nnseq_default_cfg(C.byref(cfg))
        if weight_threshold is not None:
            cfg.weight_threshold = float(weight_threshold)
        cfg.ce_smoothing_weight, cfg.frame_rejection_threshold, cfg.prior_scale = float(ce_smoothing_weight), float(frame_rejection_threshold), float(prior_scale)
        self._prior = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float32)
        if self._prior is not None and len(self._prior) != trainer.n_outputs:
            raise ValueError("SegmentwiseNnTrainer: log_prior has %d entries, the network %d outputs" % (len(self._prior), trainer.n_outputs))
        cfg.log_prior = _ptr(self._prior)
        cfg.full_batch, cfg.accumulate_prior = int(bool(full_batch)), int(bool(accumulate_prior))
        cfg.label_type = 0 if label_type == "emission-ids" else 1
        cfg.keep_lattice_error = int(bool(keep_lattice_error))
        h = C.c_void_p()
        _lib.check(self.L.amx_nnseq_create(trainer.h, C.byref(cfg), C.byref(h)))
        self.h, self.n_seg = h, 0

    def close(self):
        if self.h:
            self.L.amx_nnseq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def kernel_shape():
        """dict(sort_block_items, score_block_arcs, score_stage_items, threads)"""
        v = [C.c_int() for _ in range(4)]
        _lib.lib().amx_nnseq_kernel_shape(*(C.byref(x) for x in v))
        return dict(zip(("sort_block_items", "score_block_arcs", "score_stage_items", "threads"), (x.value for x in v)))

    @staticmethod
    def _tables(t, who):
        try:
            return (np.ascontiguousarray(t["arc_offsets"], dtype=np.int64), np.ascontiguousarray(t["item_offsets"], dtype=np.int64),
                    np.ascontiguousarray(t["item_frame"], dtype=np.int32), np.ascontiguousarray(t["item_emission"], dtype=np.int32))
        except KeyError as e:
            raise ValueError("%s: the arc tables lack %s" % (who, e))

    def forward_dev(self, feats_dev, feats_stride, frame_offsets):
        """feats_dev f32 [rows x feats_stride] on the device; segment s owns the rows [frame_offsets[s], frame_offsets[s + 1])"""
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        _lib.check(self.L.amx_nnseq_forward_dev(self.h, _ptr(feats_dev), int(feats_stride), len(off) - 1, _ptr(off)))
        self.n_seg, self.frame_offsets = len(off) - 1, off

    def arc_scores_dev(self, tables, arc_score_dev):
        """EmissionLatticeRescorer's acoustic arc scores into arc_score_dev f32 [n_arcs] (device)"""
        ao, io, fr, em = self._tables(tables, "SegmentwiseNnTrainer.arc_scores_dev")
        if len(ao) != self.n_seg + 1 or len(io) != int(ao[-1]) + 1 or len(fr) != int(io[-1]) or len(em) != len(fr):
            raise ValueError("SegmentwiseNnTrainer.arc_scores_dev: the arc tables do not fit the %d segments of the forward pass" % self.n_seg)
        _lib.check(self.L.amx_nnseq_arc_scores_dev(self.h, _ptr(ao), _ptr(io), _ptr(fr), _ptr(em), _ptr(arc_score_dev)))

    def arc_scores(self, tables):
        import torch
        n = int(np.asarray(tables["arc_offsets"])[-1])
        out = torch.zeros(max(n, 1), dtype=torch.float32, device=torch.device("cuda", self.ctx.device))
        torch.cuda.synchronize()
        self.arc_scores_dev(tables, out)
        return out[:n]

    def accumulate_dev(self, passes, emission_dev, objective, acc_dev, skip=None):
        """passes: list of dict(tables=..., arc_weight_dev=f32 device tensor [n_arcs], factor=+-1.0, negate=False, role="add" |
        "reject" | "reject-clear"); emission_dev u32 [frames] from frame_offsets[0] on (0xffffffff: no alignment); objective f32 [n_seg]
        (host); skip [n_seg] or None.  -> dict(segments_processed, segments_skipped, segments_without_alignment, observations,
        rejected_observations, ce_objective, seg_reason, seg_errors, seg_rejected, seg_ce_objective)"""
        who, n = "SegmentwiseNnTrainer.accumulate_dev", self.n_seg
        arr, keep = (_lib.NnSeqPass * max(len(passes), 1))(), []
        for k, p in enumerate(passes):
            ao, io, fr, em = self._tables(p["tables"], who)
            if len(ao) != n + 1 or len(io) != int(ao[-1]) + 1 or len(fr) != int(io[-1]) or len(em) != len(fr):
                raise ValueError("%s: pass %d: the arc tables do not fit the %d segments of the forward pass" % (who, k, n))
            w = p["arc_weight_dev"]
            if int(ao[-1]) and (w is None or w.numel() < int(ao[-1])):
                raise ValueError("%s: pass %d: arc_weight_dev holds fewer than %d weights" % (who, k, int(ao[-1])))
            keep.append((ao, io, fr, em, w))
            arr[k] = _lib.NnSeqPass(_ptr(ao), _ptr(io), _ptr(fr), _ptr(em), _ptr(w), int(bool(p.get("negate", False))), float(p.get("factor", 1.0)),
                                    self.ROLES[p.get("role", "add")])
        obj = np.ascontiguousarray(objective, dtype=np.float32)
        sk = None if skip is None else np.ascontiguousarray(skip).astype(np.uint8)
        if len(obj) != n or (sk is not None and len(sk) != n):
            raise ValueError("%s: objective and skip need one entry per segment (%d)" % (who, n))
        info = _lib.NnSeqInfo()
        out = dict(seg_reason=np.zeros(n, np.int32), seg_errors=np.zeros(n, np.uint32), seg_rejected=np.zeros(n, np.uint32), seg_ce_objective=np.zeros(n, np.float32))
        for k, v in out.items():
            setattr(info, k, _ptr(v))
        _lib.check(self.L.amx_nnseq_accumulate_dev(self.h, len(passes), C.cast(arr, C.c_void_p), _ptr(emission_dev), _ptr(sk), _ptr(obj), _ptr(acc_dev), C.byref(info)))
        for k in ("segments_processed", "segments_skipped", "segments_without_alignment", "observations", "rejected_observations", "ce_objective"):
            out[k] = getattr(info, k)
        return out

    # ---- diagnostics
    def workspace_row(self, segment):
        r = C.c_int()
        _lib.check(self.L.amx_nnseq_workspace_row(self.h, int(segment), C.byref(r)))
        return r.value

    def _segment_rows(self, segment):
        return self.workspace_row(segment), int(self.frame_offsets[segment + 1] - self.frame_offsets[segment])

    def top(self, segment, softmax=False):
        """[frames x n_outputs] of a segment: the linear top output, or the softmax p the smoothing left"""
        r, n = self._segment_rows(segment)
        out = np.zeros((n, self.trainer.n_outputs), np.float32)
        _lib.check(self.L.amx_nnseq_get_top(self.h, int(bool(softmax)), r, n, _ptr(out)))
        return out

    def error_signal(self, segment, layer=None):
        """[frames x out_dim] of a segment; layer None: the top layer's; "lattice": the copy keep_lattice_error keeps"""
        r, n = self._segment_rows(segment)
        lay = self.trainer.layout
        l = -1 if layer == "lattice" else (lay.n_layers - 1 if layer is None else int(layer))
        out = np.zeros((n, lay.n_outputs if l < 0 else lay.out_dim[l]), np.float32)
        _lib.check(self.L.amx_nnseq_get_error_signal(self.h, l, r, n, _ptr(out)))
        return out

    def weights(self, segment):
        r, n = self._segment_rows(segment)
        out = np.zeros(n, np.float32)
        _lib.check(self.L.amx_nnseq_get_weights(self.h, r, n, _ptr(out)))
        return out

    def last_shape(self):
        a, b = C.c_int(), C.c_int()
        _lib.check(self.L.amx_nnseq_last_shape(self.h, C.byref(a), C.byref(b)))
        return dict(sort_passes=a.value, sort_blocks=b.value)
