/*
 * amx.h -- C ABI of librasr_amd.so: MI355X (gfx950) acoustic front-end and emission scorers
 * for RASR.  Plain C, no RASR / torch types.  This is the drop-in boundary: the RASR-side
 * adapters subclass Flow::Node and Mm::FeatureScorer and forward to these
 * entry points; nothing else of RASR is replaced.
 *
 * Reference interfaces replaced (paths relative to /root/reference/src):
 *   amx_mfcc_*   the Flow sub-network Tools/FeatureExtraction/share/mfcc.flow:8-34, i.e. the nodes
 *                Signal/Preemphasis.cc:108-124, Signal/SlidingAlgorithmNode.hh:60-79 (signal-window),
 *                Signal/FastFourierTransform.hh:311-320, Signal/ComplexVectorFunction.hh:234-243,
 *                Signal/Filterbank.cc:860-876, Flow/SimpleFunction.hh:497-507,
 *                Signal/CosineTransform.cc:213-228 -- driven per segment by
 *                Speech/DataExtractor.cc:101-111 (FeatureExtractor::processSegment).
 *   amx_gmm_*    Mm::FeatureScorer::getScorer(x)->score(e) as implemented by
 *                Mm/GaussDiagonalMaximumFeatureScorer.cc:116-141 (max) and :252-298 (log-add),
 *                constructed by Mm/FeatureScorerFactory.hh:72-82 from a Mm::MixtureSet.
 *   amx_ffnn_*   Nn::BatchFeatureScorer (Nn/BatchFeatureScorer.cc:45-171): forward of
 *                Nn::NeuralNetwork<f32> (Nn/NeuralNetwork.cc:313-331) with the softmax disabled and
 *                the scaled log-prior removed from the output bias; score = -activation.
 *   amx_stats_*  the per-partition accumulator files + `combine-mixture-set-estimators`
 *                (Tools/AcousticModelTrainer/AcousticModelTrainer.cc:317-325) -- here a flat device
 *                buffer the caller all-reduces (RCCL) once per epoch.
 *
 * Conventions
 *   - every function returns an amx_status (0 = ok, < 0 = error); amx_last_error() gives the
 *     thread-local message of the last failure.  Nothing exits or throws across the boundary.
 *   - "host" pointers are ordinary process memory (pinned recommended); "dev" pointers are HBM
 *     addresses on the context's device (hipMalloc / torch tensor data_ptr).
 *   - all matrices handed over the boundary are row-major [frames x dim] f32.
 *   - scores are negative log-likelihoods (Mm::Score = f32, smaller is better).
 *   - a context is bound to one device and one HIP stream; calls on one context must be
 *     externally serialised (RASR's corpus loop is single threaded, Speech/Recognizer.cc:271-281).
 */
#ifndef RASR_AMD_AMX_H
#define RASR_AMD_AMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    AMX_OK              = 0,
    AMX_ERR_INVALID     = -1, /* bad argument / configuration (reference would criticalError) */
    AMX_ERR_UNSUPPORTED = -2, /* valid RASR configuration this build has no kernel for */
    AMX_ERR_DEVICE      = -3, /* HIP runtime failure, no gfx950 device, out of memory */
    AMX_ERR_STATE       = -4  /* call sequence violates the protocol (reference would require()) */
} amx_status;

typedef struct amx_ctx  amx_ctx;
typedef struct amx_mfcc amx_mfcc;
typedef struct amx_mfcc_plan amx_mfcc_plan;
typedef struct amx_gmm  amx_gmm;
typedef struct amx_ffnn amx_ffnn;

/* ------------------------------------------------------------------ context */

/* "rasr_amd <version> (gfx950; <compiler>; <flags>; src=<12 hex digits>)": the source hash is the SHA-1 of the files of rasr_amd/csrc/ and
 * include/amx.h the library was built from (rasr_amd/csrc/Makefile), so that a measurement can be tied to a build. */
const char* amx_version(void);
const char* amx_last_error(void);
/* Creates a context on HIP device `device_ordinal` with its own non-blocking stream. */
int  amx_init(int device_ordinal, amx_ctx** out);
void amx_destroy(amx_ctx* ctx);
/* Run all subsequent launches of this context on the caller's hipStream_t (e.g. torch's current
 * stream); NULL restores the context's own stream.  To run on the legacy default stream pass hipStreamLegacy
 * ((hipStream_t)1): the handle 0 that frameworks report for it would read as NULL here. */
int amx_set_stream(amx_ctx* ctx, void* hip_stream);
int amx_synchronize(amx_ctx* ctx);

/* WHICH BUILD OF THE REFERENCE this context's f32 arithmetic follows (round 6; cmake_resources/CompileOptions.cmake:21-48).  RASR has
 * two arithmetics, decided by how it was compiled:
 *   AMX_CONTRACT_OFF  -DMARCH=x86-64 (or a host / compiler without fused multiply-adds): every product and every sum rounds once;
 *   AMX_CONTRACT_FMA  its DEFAULT configuration, -march=native on an FMA host with GCC (-ffp-contract=fast; clang's default `on` fuses
 *                     within a statement: treat clang builds as FMA too): `sum += a * b` is ONE fused multiply-add at the sites
 *                     oracle/orc.h marks ORC_FMAF / ORC_FMA -- the GMM distance (Mm/GaussDiagonalMaximumFeatureScorer.cc:144-218,
 *                     Mm/BatchFeatureScorer.cc:164-650), Signal::Regression (Signal/Regression.cc:24-65), Math::Vector's dot product
 *                     (Math/Vector.hh:94-101: signal-matrix-multiplication-f32, the cosine transform), Filter::apply
 *                     (Signal/Filterbank.cc:27-50), preemphasis with alpha != 1, the filter bank's geometry, the AR-to-cepstrum
 *                     recursion, the gammatone design / cascade / integrations, the amplitude-spectrum-energy normalisation.
 * The setting is read (a) by every *_dev entry point that takes the context directly (amx_regression_dev, amx_matrix_multiply_dev,
 * amx_vector_normalize_dev, ...) at call time, (b) by amx_mfcc_create / amx_gammatone_create / amx_gmm_create at creation (a handle
 * keeps the arithmetic it was created with; amx_gmm_model.tuning "contract=off|fma" overrides it per model).  Default: OFF.
 * An adapter compiled INSIDE RASR's build knows the answer at compile time: pass AMX_CONTRACT_OF_THIS_BUILD right after amx_init --
 * the macro is evaluated in the translation unit that includes this header, i.e. with RASR's own flags.
 * Bit-exact against oracle/liboracle.so (OFF) / oracle/liboracle_fma.so (FMA) wherever the OFF arithmetic is (tests/test_contract_gpu.py). */
enum { AMX_CONTRACT_OFF = 0, AMX_CONTRACT_FMA = 1 };
#if defined(__FMA__) && (defined(__GNUC__) || defined(__clang__)) && !defined(AMX_ADAPTER_NO_FP_CONTRACT)
#define AMX_CONTRACT_OF_THIS_BUILD AMX_CONTRACT_FMA /* -mfma / -march=native on an FMA host, GCC or clang defaults (define AMX_ADAPTER_NO_FP_CONTRACT when RASR is built with -ffp-contract=off) */
#else
#define AMX_CONTRACT_OF_THIS_BUILD AMX_CONTRACT_OFF
#endif
int amx_set_contract(amx_ctx* ctx, int contract);
int amx_get_contract(const amx_ctx* ctx); /* AMX_CONTRACT_OFF | AMX_CONTRACT_FMA; < 0: ctx is NULL */
/* "contract=off: RASR built with -DMARCH=x86-64 ..." -- one line an adapter logs next to the reference's own "Scaling factor" lines */
const char* amx_contract_description(int contract);
/* Per-kernel timing with HIP events on the context's stream (used by bench.py for the roofline
 * line).  enable=1 makes every launch of the named hot kernels record start/stop events. */
int amx_profile_enable(amx_ctx* ctx, int enable);
int amx_profile_reset(amx_ctx* ctx);
/* kernel: "mfcc", "gmm", "gmm_dist", "gmm_combine", "ffnn_gemm" (all layers), "ffnn_gemm_max"
 * (largest layer only).  Synchronises the stream.  avg_ms = mean launch duration. */
int amx_profile_get(amx_ctx* ctx, const char* kernel, double* avg_ms, long* n_launches);

/* ------------------------------------------------------------------ MFCC front-end */

typedef struct {
    double sample_rate;            /* Hz */
    double win_len_s;              /* signal-window length        (mfcc.flow: 0.025) */
    double win_shift_s;            /* signal-window shift         (mfcc.flow: 0.01)  */
    double preemph_alpha;          /* signal-preemphasis alpha    (mfcc.flow: 1.00)  */
    double fft_max_input_s;        /* maximum-input-size          (mfcc.flow: 0.025) */
    int    apply_scale;            /* apply-scale, default 1: spectrum * 1/(f32)fs   */
    double mel_filter_width;       /* filter-width, default 268.258 (mel)            */
    double mel_spacing;            /* spacing, default 0 => 0.5 * width              */
    int    warp_differential_unit; /* warp-differential-unit, default 1              */
    int    n_ceps;                 /* signal-cosine-transform nr-outputs             */
    int    dct_normalize;          /* normalize, default 0                           */
    /* front_end AMX_FRONT_END_MFPLP = mfplp.flow (Tools/FeatureExtraction/share/mfplp.flow:9-47): amplitude ->
     * generic-vector-f32-power 2 -> mel filter bank -> generic-vector-f32-power plp_power -> signal-cosine-transform
     * (input-type N-plus-one, nr-outputs n_autocorrelation, normalize) -> signal-autocorrelation-to-autoregression
     * (Math/LevinsonLse.cc:35-70) -> signal-autoregression-to-cepstrum (Signal/AutoregressionToCepstrum.cc:21-35,
     * nr-outputs n_ceps).  A frame whose Levinson recursion meets a zero prediction error (digital silence) is an error in
     * the reference ("Failed to calculate the autoregression coefficients."); it comes out as NaNs here. */
    int    front_end;              /* AMX_FRONT_END_MFCC (0, default), AMX_FRONT_END_MFPLP or AMX_FRONT_END_PLP  */
    int    n_autocorrelation;      /* nr-autocorrelation-coefficients = LPC order + 1 (MF-PLP, PLP)                */
    double plp_power;              /* intensity-loudness-law value, default 0.33 (MF-PLP, PLP)                     */
    /* The other parameters of signal-filterbank (Signal/Filterbank.cc:700-745), usable with every front end; the defaults (0) are
     * mfcc.flow's.  warp-center-positions stays true (the reference's default; stretch-to-cover accepts nothing else).
     * front_end AMX_FRONT_END_PLP = plp.flow (Tools/FeatureExtraction/share/plp.flow): Hamming 20 ms, no preemphasis node
     * (preemph_alpha 0), power spectrum -> trapeze / include-boundary / bark filter bank (filter-width 3.8, spacing 0.93853 = 20
     * filters at 16 kHz; 0.973442 = 15 filters at 8 kHz) -> the vector extended by copies of its first and last element
     * (generic-vector-f32-split / -concat) -> equal-loudness preemphasis (signal-vector-f32-continuous-transform,
     * Signal/VectorTransform.cc:36-83, f = equal-loudness(bark^-1(index / sample-rate)), operation multiplies) -> ^plp_power ->
     * the MF-PLP tail (cosine transform N-plus-one, Levinson, LPC cepstrum). */
    int    filter_type;            /* type: AMX_FILTER_TRIANGULAR (0) or AMX_FILTER_TRAPEZE                        */
    int    boundary;               /* boundary: AMX_BOUNDARY_STRETCH_TO_COVER (0), _INCLUDE, _EMPHASIZE            */
    int    warping;                /* warping-function: AMX_WARP_MEL (0) or AMX_WARP_BARK                          */
    /* Kernel selection for A/B runs and tests, "key=value,key=value" (NULL: defaults; an unknown key fails amx_mfcc_create).  None
     * of them changes a result beyond the parity bars.  fft=stockham|mfma|r16 (LDS radix-4 butterflies | the 256-point transform as
     * two matrix products | radix-16 register butterflies, four frames per wave: mfcc.flow with a 512-point transform only),
     * prefetch=1|0 (a wave fetches its next frame's samples while it transforms the current one; default 1), wgs=N (workgroups
     * per CU), lpc=regs|lds (LPC-cepstrum recursion in registers | the LDS kernel). */
    const char* tuning;
} amx_mfcc_cfg;
enum { AMX_FRONT_END_MFCC = 0, AMX_FRONT_END_MFPLP = 1, AMX_FRONT_END_PLP = 2 };
enum { AMX_FILTER_TRIANGULAR = 0, AMX_FILTER_TRAPEZE = 1 };
enum { AMX_BOUNDARY_STRETCH_TO_COVER = 0, AMX_BOUNDARY_INCLUDE = 1, AMX_BOUNDARY_EMPHASIZE = 2 };
enum { AMX_WARP_MEL = 0, AMX_WARP_BARK = 1 };

typedef struct {
    int    frame_len, frame_shift, fft_len, n_bins, n_filters, n_ceps;
    double fft_output_sample_rate; /* attribute "sample-rate" after the FFT node = N/fs */
    double mel_max;                /* warped maximum frequency */
    int    n_transform;            /* rows of the cosine-transform table: n_ceps (MFCC) or n_autocorrelation (MF-PLP, PLP) */
    int    n_transform_inputs;     /* its columns: n_filters, or n_filters + 2 (PLP: first and last filter output duplicated) */
} amx_mfcc_info;

void amx_mfcc_default_cfg(amx_mfcc_cfg* cfg); /* the values of mfcc.flow + node defaults, 16 ceps */
void amx_mfplp_default_cfg(amx_mfcc_cfg* cfg); /* the values of mfplp.flow, 13 autocorrelation / 13 cepstrum coefficients */
void amx_plp_default_cfg(amx_mfcc_cfg* cfg);   /* the values of plp.flow at 16 kHz, 13 autocorrelation / 13 cepstrum coefficients */
int  amx_mfcc_create(amx_ctx* ctx, const amx_mfcc_cfg* cfg, amx_mfcc** out);
void amx_mfcc_destroy(amx_mfcc* h);
int  amx_mfcc_describe(const amx_mfcc* h, amx_mfcc_info* info);
/* frames produced for a segment of n_samples (framing + flush rule of Signal/WindowBuffer.cc:84-125) */
long amx_mfcc_n_frames(const amx_mfcc* h, long n_samples);
/* start time of frame k relative to the segment start, accumulated exactly like
 * WindowBuffer::get (bufferStartTime_ += shift / sampleRate) */
double amx_mfcc_frame_start_time(const amx_mfcc* h, long frame);
/* host copies of the tables the kernel uses (any pointer may be NULL):
 * window[frame_len], filter_start/end[n_filters], filter_offset[n_filters+1],
 * filter_weights[filter_offset[n_filters]], dct[n_transform*n_transform_inputs] */
int amx_mfcc_tables(const amx_mfcc* h, float* window, int* filter_start, int* filter_end,
                    int* filter_offset, float* filter_weights, float* dct);
/* PLP: the equal-loudness factors [n_transform_inputs] (f64, as the reference's f(i)); AMX_ERR_STATE for the other front ends */
int amx_mfcc_equal_loudness(const amx_mfcc* h, double* factors);

/* One segment, host buffers: pcm f32 (s16 sample values, unscaled, Flow/TypeConverter.hh:35-43)
 * -> ceps [n_frames x n_ceps].  Includes H2D/D2H. */
int amx_mfcc_run(amx_mfcc* h, const float* pcm_host, long n_samples, float* ceps_host);
/* Batch of segments, host buffers. */
int amx_mfcc_run_batch(amx_mfcc* h, int n_seg, const float* const* pcm_host, const long* n_samples,
                       float* const* ceps_host);
/* The same with the samples as the audio file holds them: s16, widened to f32 without scaling inside the kernel exactly like the
 * converter node in front of the chain (Flow/TypeConverter.hh:35-43) -- 320 instead of 640 bytes per frame over the host link and
 * out of HBM; results are bit-identical to the f32 entry points on the same sample values. */
int amx_mfcc_run_s16(amx_mfcc* h, const int16_t* pcm_host, long n_samples, float* ceps_host);
int amx_mfcc_run_batch_s16(amx_mfcc* h, int n_seg, const int16_t* const* pcm_host, const long* n_samples,
                           float* const* ceps_host);

/* Device-resident batches.  A plan fixes the segmentation: segment u occupies samples
 * [sample_offsets[u], sample_offsets[u+1]) of one concatenated PCM buffer and frames
 * [frame_offsets[u], frame_offsets[u+1]) of one [total_frames x n_ceps] output. */
int  amx_mfcc_plan_create(amx_mfcc* h, int n_seg, const long* sample_offsets /*[n_seg+1]*/, amx_mfcc_plan** out);
void amx_mfcc_plan_destroy(amx_mfcc_plan* p);
long amx_mfcc_plan_total_frames(const amx_mfcc_plan* p);
int  amx_mfcc_plan_frame_offsets(const amx_mfcc_plan* p, long* frame_offsets /*[n_seg+1]*/);
int  amx_mfcc_run_plan_dev(amx_mfcc* h, const amx_mfcc_plan* p, const float* pcm_dev, float* ceps_dev);
int  amx_mfcc_run_plan_dev_s16(amx_mfcc* h, const amx_mfcc_plan* p, const int16_t* pcm_dev, float* ceps_dev);

/* Vocal tract length normalisation in the filter bank: signal-filterbank's
 *     warping-function = nest(linear-2($(warping-factor), limit), mel)      (bark for PLP)
 * (Signal/Filterbank.cc:798-816, Math/AnalyticFunctionFactory.cc:394-430), with the factor chosen per segment.  linear-2 is the
 * two-piece linear function of slope `factor` up to limit * fs/2 that maps fs/2 onto itself (a factor > 1: the inverse of the one
 * built for 1 / factor); it is applied in front of cfg->warping, which still selects mel or bark.  A handle holds one filter bank per
 * factor, all built and uploaded at creation; factor 1 gives the unwarped bank bit for bit.  All banks must have the same number of
 * filters (AMX_ERR_INVALID naming the two factors otherwise).  Every entry point that takes no factor (amx_mfcc_run*,
 * amx_mfcc_plan_create, amx_mfcc_tables) uses factors[0].  A plan names one of the handle's factors per segment (exactly, else
 * AMX_ERR_INVALID naming the segment); the kernel picks the bank per tile. */
#define AMX_MFCC_MAX_WARPING_FACTORS 64
typedef struct {
    double        limit;      /* linear-2's second argument, in (0, 1); RASR recipes use 0.875 */
    int           n_factors;  /* 1 .. AMX_MFCC_MAX_WARPING_FACTORS */
    const double* factors;    /* [n_factors] each finite and > 0, no duplicates; factors[0] is the handle's default */
} amx_mfcc_vtln;
int amx_mfcc_create_vtln(amx_ctx* ctx, const amx_mfcc_cfg* cfg, const amx_mfcc_vtln* vtln, amx_mfcc** out);
int amx_mfcc_plan_create_vtln(amx_mfcc* h, int n_seg, const long* sample_offsets /*[n_seg+1]*/, const double* warping_factor /*[n_seg]*/,
                              amx_mfcc_plan** out);
/* amx_mfcc_tables for the bank of one of the handle's factors (AMX_ERR_INVALID for any other factor; a handle made by
 * amx_mfcc_create has the one factor 1) */
int amx_mfcc_tables_vtln(const amx_mfcc* h, double warping_factor, float* window, int* filter_start, int* filter_end,
                         int* filter_offset, float* filter_weights, float* dct);

/* ------------------------------------------------------------------ sample stream in front of the feature chains (samples.flow)
 * signal-dc-detection (Signal::DcDetection, src/Signal/DcDetection.cc:90-235): a host-side scan over one segment's samples that tells
 * the caller which sample ranges reach the feature chain.  Runs of at least min-dc-length seconds whose samples stay within
 * max-dc-increment of the last accepted sample are dropped, and so are non-DC stretches shorter than min-non-dc-segment-length (node
 * defaults .0125 / 0.9 / .02, maximal-output-size 4096; samples.flow uses .0125 / 0.9 / .026).  max_dc_increment = 0 disables the
 * detection (every sample is accepted).  Output: the node's blocks as (first sample, length) in stream order -- merge = 0: exactly
 * the vectors the node emits; merge = 1: neighbouring blocks without a time gap joined, i.e. the ranges the window buffer behind it
 * frames without an intermediate flush (one entry of an amx_mfcc_plan's sample_offsets each).  starts / lengths may be NULL to count. */
int amx_dc_detection(const float* pcm, long long n_samples, double sample_rate, double min_dc_length_s, float max_dc_increment,
                     double min_non_dc_segment_length_s, int maximal_output_size, int merge, long long* starts, long long* lengths,
                     long long capacity, long long* n_blocks);

/* ------------------------------------------------------------------ gammatone front-end
 * The three nodes of Signal/Module.cc:169-173 -- signal-gammatone (Signal/GammaTone.cc:20-231), signal-temporalintegration
 * (Signal/TemporalIntegration.cc:60-84 over Signal/TimeWindowBuffer.cc:52-125) and signal-spectralintegration
 * (Signal/SpectralIntegration.cc:55-74) -- as one front end, PCM in, one vector per 10 ms frame out, with the usual tail
 * (generic-vector-f32-power, signal-cosine-transform) optional.  Field names are the nodes' parameter names; the defaults are the
 * nodes' own.  Temporal integration frames follow the window node's rule (short last frames, amx_gammatone_n_frames); the state
 * of the filter cascade starts at zero with every segment (the node resets at end of segment). */
typedef struct {
    double sample_rate;      /* Hz */
    int    cascade;          /* signal-gammatone cascade, default 4 (0..8)                                   */
    double min_freq;         /* minfreq, default 100                                                         */
    double max_freq;         /* maxfreq, default 6000                                                        */
    double q;                /* q, default 9.264491981582191 (the 0 Hz bandwidth l = 24.7 is not a parameter) */
    int    channels;         /* channels, default 50                                                         */
    int    cf_mode;          /* cfmode: AMX_GAMMATONE_HUMAN (0, default) or AMX_GAMMATONE_ERB                */
    double warp_freq_break;  /* warp-freqbreak, default 6600                                                 */
    double warping_factor;   /* warping-factor, default 1 (the upper end of the warping is sample_rate / 2)  */
    int    ti_window;        /* signal-temporalintegration type: AMX_WINDOW_HANNING (0) or AMX_WINDOW_RECTANGULAR */
    double ti_length_s;      /* length (seconds)                                                             */
    double ti_shift_s;       /* shift (seconds)                                                              */
    int    si_window;        /* signal-spectralintegration type                                              */
    int    si_length;        /* length in channels; 0 = node absent                                          */
    int    si_shift;         /* shift in channels                                                            */
    double power;            /* generic-vector-f32-power value (e.g. 0.1 for the 10th root); 0 = node absent */
    int    n_ceps;           /* signal-cosine-transform nr-outputs; 0 = node absent                          */
    int    dct_normalize;    /* normalize                                                                    */
    /* "contract=off|fma" (NULL: the context's arithmetic, amx_set_contract; OFF for a host-only handle): which build of the reference
     * the design (centre frequencies, warping), the filter cascade, both integrations and the cosine transform follow -- bit for bit
     * in either mode (oracle/orc_gammatone.c marks the contracted sites).  Unknown keys / values fail amx_gammatone_create. */
    const char* tuning;
} amx_gammatone_cfg;
enum { AMX_GAMMATONE_HUMAN = 0, AMX_GAMMATONE_ERB = 1 };
enum { AMX_WINDOW_HANNING = 0, AMX_WINDOW_RECTANGULAR = 1 };
typedef struct {
    int channels, cascade, frame_len, frame_shift;
    int si_channels; /* channels after spectral integration */
    int n_out;       /* output dimension */
} amx_gammatone_info;
typedef struct amx_gammatone amx_gammatone;
void amx_gammatone_default_cfg(amx_gammatone_cfg* cfg);
int  amx_gammatone_create(amx_ctx* ctx, const amx_gammatone_cfg* cfg, amx_gammatone** out); /* ctx NULL: host-only (tables, geometry) */
void amx_gammatone_destroy(amx_gammatone* h);
int  amx_gammatone_describe(const amx_gammatone* h, amx_gammatone_info* info);
long amx_gammatone_n_frames(const amx_gammatone* h, long n_samples);
/* centre frequencies [channels] and filter coefficients [channels][4] = a0, a1, b1, b2 (GammaTone::Coefficient); nullable */
int amx_gammatone_tables(const amx_gammatone* h, float* center_freq, float* coefficients);
/* one segment, host buffers: pcm f32 -> out [n_frames x n_out] */
int amx_gammatone_run(amx_gammatone* h, const float* pcm_host, long n_samples, float* out_host);
/* a batch of segments resident in HBM: segment u = samples [sample_offsets[u], sample_offsets[u+1]) of pcm_dev (offsets on the
 * host), its frames follow those of segment u - 1 in out_dev [total frames x n_out].  filtered_dev (nullable, [total samples x
 * channels]) receives the signal-gammatone node's own output. */
int amx_gammatone_run_batch_dev(amx_gammatone* h, int n_seg, const long* sample_offsets, const float* pcm_dev, float* out_dev,
                                float* filtered_dev);

/* ------------------------------------------------------------------ voicedness front-end
 * Tools/FeatureExtraction/share/voicedness.flow as one front end, PCM in, ONE f32 per 10 ms frame out: signal-window (rectangular;
 * Signal/TimeWindowBuffer.cc:52-125, short last frame included) -> signal-vector-f32-resize (Signal/VectorResize.hh:93-113: the short
 * frame padded with zeros to the window length) -> signal-vector-f32-mean-energy-normalization (Signal/VectorNormalization.hh:44-49)
 * -> signal-cross-correlation with x = y (Signal/CrossCorrelation.cc:31-64, 111-127, 225-243; CrossCorrelation.hh:33-49: real FFT of
 * length next-pow-2(size + end - 1), X conj(X), real inverse FFT, lags [0, end), unbiased estimate R[m] / (size - m)) ->
 * signal-peak-detection, output maximal-peak-value (Signal/PeakDetection.cc:42-68, 92-98, 252-277).
 * Built: sample rates whose 40 ms window needs a 1024- or 2048-point transform (8 kHz, 16 kHz), begin = 0, similarity-function =
 * multiplication, use-fft = true, normalization none | unbiased-estimate.  Refused with AMX_ERR_UNSUPPORTED and a message naming the
 * parameter: begin != 0 (negative or skipped lags), normalization = upper-bound, any other transform length.  Not expressible here, so
 * an adapter refuses them itself: x != y, similarity-function = absolute-difference, use-fft = false, nr-coefficients, the other
 * seven outputs of the peak node (INTEGRATION.md has the table).
 * FRAME COUNT: the 40 ms window flushes later than mfcc.flow's 25 ms window, so a segment can yield a different number of frames than
 * its cepstra (amx_voicedness_n_frames vs amx_mfcc_n_frames); the library trims nothing -- INTEGRATION.md says how the reference's
 * timestamp synchronisation lines the two streams up.
 * The normalisation is the same in both builds of the reference (its two builds give the same bits on the recorded frames,
 * tests/golden/ref_voicedness.npz; the f32 product is converted before the f64 add) and the kernel's energy sum is the index-order
 * sum bit for bit (amx_voicedness_energy_dev).  The two builds differ in X conj(X), an f32 site; the device transforms are f32 and
 * agree with either build within the front-end bar (DESIGN.md sections 4.6 and 5). */
typedef struct {
    double sample_rate;     /* Hz */
    double win_len_s;       /* signal-window length = signal-vector-f32-resize new-size (voicedness.flow: .040) */
    double win_shift_s;     /* signal-window shift                                       (voicedness.flow: .010) */
    double corr_begin_s;    /* signal-cross-correlation begin: 0 only                                           */
    double corr_end_s;      /* signal-cross-correlation end                              (voicedness.flow: .040) */
    int    normalization;   /* AMX_XCORR_NONE | AMX_XCORR_UNBIASED_ESTIMATE (voicedness.flow); _UPPER_BOUND is refused */
    double min_position_s;  /* signal-peak-detection min-position                       (voicedness.flow: .0025) */
    double max_position_s;  /* signal-peak-detection max-position                       (voicedness.flow: .0167) */
    const char* tuning;     /* NULL; no keys yet (an unknown key fails amx_voicedness_create)                   */
} amx_voicedness_cfg;
enum { AMX_XCORR_NONE = 0, AMX_XCORR_UNBIASED_ESTIMATE = 1, AMX_XCORR_UPPER_BOUND = 2 };
typedef struct {
    int frame_len, frame_shift, fft_len;
    int n_lags;                     /* end - begin: the length of the autocorrelation vector the peak node sees */
    int min_position, max_position; /* as indices: (u32)rint(seconds * sample rate), PeakDetection::init         */
} amx_voicedness_info;
typedef struct amx_voicedness amx_voicedness;
void amx_voicedness_default_cfg(amx_voicedness_cfg* cfg); /* voicedness.flow at 16 kHz */
int  amx_voicedness_create(amx_ctx* ctx, const amx_voicedness_cfg* cfg, amx_voicedness** out); /* ctx NULL: host-only (geometry) */
void amx_voicedness_destroy(amx_voicedness* h);
int  amx_voicedness_describe(const amx_voicedness* h, amx_voicedness_info* info);
/* frames of a segment of n_samples: the window node's framing and flush rule (Signal/WindowBuffer.cc:84-125) with the 40 ms window */
long amx_voicedness_n_frames(const amx_voicedness* h, long n_samples);
/* one segment, host buffers: pcm f32 -> out [n_frames] */
int amx_voicedness_run(amx_voicedness* h, const float* pcm_host, long n_samples, float* out_host);
/* a batch of segments resident in HBM: segment u = samples [sample_offsets[u], sample_offsets[u+1]) of pcm_dev (offsets on the
 * host), its frames follow those of segment u - 1.  Frame t's measure is written to out_dev[t * out_ld] and nothing else is: out_ld
 * is a row stride in floats, so out_dev may be one column of a wider feature matrix.  acf_dev (nullable, tests: [total frames x
 * n_lags]) receives the normalised autocorrelation the peak detection saw.  _s16: the samples as the audio file holds them, widened
 * without scaling (Flow/TypeConverter.hh:35-43); bit-identical to the f32 entry point on the same sample values. */
int amx_voicedness_run_batch_dev(amx_voicedness* h, int n_seg, const long* sample_offsets, const float* pcm_dev, float* out_dev, int out_ld,
                                 float* acf_dev);
int amx_voicedness_run_batch_dev_s16(amx_voicedness* h, int n_seg, const long* sample_offsets, const int16_t* pcm_dev, float* out_dev,
                                     int out_ld, float* acf_dev);

/* Test-only: the energy sum of the normalisation (std::inner_product over the resized frame, VectorNormalization.hh:45) of every frame
 * as the kernel forms it, [total frames] f64, and how it was added: ordered_dev[t] = 0 in lane order (proved exact in any order), 1 by
 * one lane in index order. */
int amx_voicedness_energy_dev(amx_voicedness* h, int n_seg, const long* sample_offsets, const float* pcm_dev, double* sum_dev, int* ordered_dev);

/* Sliding-window concatenation of feature frames per segment (f1 "next" row:
 * signal-vector-f32-sequence-concatenation, Signal/SlidingWindow.hh:66-76 copy margin policy):
 * out[t] = [x[t-left] .. x[t+right]] with indices clamped to the segment.  out_dev is
 * [total_frames x out_stride] f32 (out_stride >= (left+right+1)*dim, padding zero-filled). */
int amx_context_window_dev(amx_ctx* ctx, const amx_mfcc_plan* p, const float* feats_dev, int dim,
                           int left, int right, float* out_dev, int out_stride);

/* Feature back-end between the front-end and the scorers, on device-resident
 * [total_frames x ld] f32 matrices segmented like the plan.  in/out may point into wider matrices (column offset by
 * pointer arithmetic, row stride *_ld), which is how "generic-vector-f32-concat" of features and derivatives is laid out.
 * Aliasing: the input and output views must not share memory -- disjoint column ranges of one wide matrix are fine, anything
 * else is rejected with AMX_ERR_INVALID; the one exception is whole-segment normalisation (length = 0) in place on the
 * identical view.
 *
 * signal-normalization (src/Signal/Normalization.cc:46-66,120-187): per segment, type mean or mean-and-variance;
 * length = 0: whole segment (length="infinite" right="infinite"); otherwise a sliding window of `length` frames with the
 * output point `right` frames from its newest end (0 <= right < length), statistics kept as the reference's running
 * f64 sums (the last `right` frames of a segment leave with the statistics of the last window, as in the reference). */
#define AMX_NORM_MEAN 0
#define AMX_NORM_MEAN_AND_VARIANCE 1
int amx_normalize_dev(amx_ctx* ctx, const amx_mfcc_plan* plan, const float* in_dev, int in_ld, int dim, int type,
                      int length, int right, float* out_dev, int out_ld);
/* the node's other types on the same window skeleton (src/Signal/Normalization.cc:100-110,196-262; NormalizationNode `type` /
 * `level`): divide-by-mean (x / mean; the reference stops with "One of the mean components is zero." where this yields inf or
 * NaN), level (out[level] = x[level] - max over the window, other components unchanged) and mean-and-variance-1D (one mean and
 * standard deviation over all components of the window).  type mean / mean-and-variance are forwarded to amx_normalize_dev. */
#define AMX_NORM_DIVIDE_BY_MEAN 2
#define AMX_NORM_LEVEL 3
#define AMX_NORM_MEAN_AND_VARIANCE_1D 4
int amx_normalize_ex_dev(amx_ctx* ctx, const amx_mfcc_plan* plan, const float* in_dev, int in_ld, int dim, int type, int level,
                         int length, int right, float* out_dev, int out_ld);
/* signal-vector-f32-{amplitude-spectrum-energy,energy,maximum,mean-energy,mean,variance}-normalization
 * (src/Signal/VectorNormalization.hh:31-163, registered in src/Signal/Module.cc:108-113): every vector on its own -- divided by
 * sqrt of its (Parseval / plain / mean) energy or by its maximum, or shifted to zero mean (and scaled to unit deviation).  A zero
 * statistic gives inf / NaN like the reference's unguarded division.  [n_vectors x dim] views with row strides; in place is
 * allowed on the identical view. */
enum { AMX_VNORM_AMPLITUDE_SPECTRUM_ENERGY = 0, AMX_VNORM_ENERGY = 1, AMX_VNORM_MAXIMUM = 2, AMX_VNORM_MEAN_ENERGY = 3, AMX_VNORM_MEAN = 4,
       AMX_VNORM_VARIANCE = 5 };
int amx_vector_normalize_dev(amx_ctx* ctx, int type, const float* in_dev, int in_ld, long n_vectors, int dim, float* out_dev, int out_ld);
/* generic-vector-f32-<function> (Flow::SimpleFunctionNode over src/Flow/SimpleFunction.hh:40-345; e.g. the x 500 scaling and the
 * quantisation of mfcc.standard_system.flow, the power nodes of mfplp.flow): one parameter, every element on its own.  Addition,
 * multiplication, quantize (rint(v / p) * p; rint(v) for p = 1 or 0), abs, minimum, maximum, sqrt and power (the node's unqualified
 * pow on floats = ::pow(double, double) narrowed) follow the reference's arithmetic exactly; log (log10), log-plus (log10(v + p)), ln,
 * exp and cos are the device's f32 functions, a few ulp from glibc's.  Views and in-place rule as for amx_vector_normalize_dev. */
enum { AMX_VFUNC_LOG = 0, AMX_VFUNC_LOG_PLUS = 1, AMX_VFUNC_LN = 2, AMX_VFUNC_EXP = 3, AMX_VFUNC_POWER = 4, AMX_VFUNC_SQRT = 5, AMX_VFUNC_COS = 6,
       AMX_VFUNC_ADDITION = 7, AMX_VFUNC_MULTIPLICATION = 8, AMX_VFUNC_QUANTIZE = 9, AMX_VFUNC_ABS = 10, AMX_VFUNC_MINIMUM = 11,
       AMX_VFUNC_MAXIMUM = 12 };
int amx_vector_function_dev(amx_ctx* ctx, int kind, float parameter, const float* in_dev, int in_ld, long n_vectors, int dim, float* out_dev,
                            int out_ld);
/* signal-delay (max-size = 2*right+1, margin-policy copy, margin-condition present-not-empty; src/Signal/Delay.hh:33-47)
 * + signal-regression order 1 or 2 (src/Signal/Regression.cc:25-68), as wired in derivationWithRegression.flow. */
int amx_regression_dev(amx_ctx* ctx, const amx_mfcc_plan* plan, const float* in_dev, int in_ld, int dim, int order,
                       int right, float* out_dev, int out_ld);
/* signal-matrix-multiplication-f32 (src/Signal/MatrixMult.hh:246-255; LDA in lda.flow): out[t] = M in[t], M [rows x cols]
 * row-major on the device (read the file with amx_nn_matrix_read: same binary Math::Matrix<f32> format). */
int amx_matrix_multiply_dev(amx_ctx* ctx, const float* matrix_dev, int rows, int cols, const float* in_dev, int in_ld,
                            int T, float* out_dev, int out_ld);

/* ------------------------------------------------------------------ diagonal-covariance GMM */

typedef struct {
    int dim, n_mix, n_dens, n_mean, n_cov;
    const uint32_t* mix_offsets; /* [n_mix+1]  mixture m owns entries [mix_offsets[m], mix_offsets[m+1]) */
    const uint32_t* dens_index;  /* [mix_offsets[n_mix]]  density index (Mm::Mixture::densityIndex) */
    const double*   log_weight;  /* [mix_offsets[n_mix]]  log weights (Mm::Weight = f64) */
    const uint32_t* dens_mean;   /* [n_dens]  Mm::GaussDensity::meanIndex */
    const uint32_t* dens_cov;    /* [n_dens]  Mm::GaussDensity::covarianceIndex */
    const float*    means;       /* [n_mean x dim] */
    const float*    variances;   /* [n_cov  x dim] diagonal variances */
    double          mixture_weight_scale; /* mixture-weight-scale (Core::ParameterFloat = f64; the scorer keeps it as f32), default 1 */
    double          gaussian_scale;       /* gaussian-scale (f64; the scorer keeps (f32)sqrt of the f64 value,
                                           * Mm/GaussDiagonalMaximumFeatureScorer.cc:52), default 1 */
    /* "key=value,key=value" (NULL: defaults).  Keys AND values are checked by amx_gmm_create -- an unknown key, a number that is not one,
     * a value the key does not take fail the creation (AMX_ERR_INVALID): a typo must not silently select another kernel or arithmetic.
     * Read by amx_gmm_create only (amx_pms_write, amx_gmm_estimate, amx_prior_from_mixture_set ignore it).
     *
     * contract=off|fma -- WHICH BUILD OF THE REFERENCE the scorer follows (without the key: the context's, amx_set_contract -- OFF unless
     *   the adapter said otherwise; see there for what the two builds are):
     *   off  RASR configured with -DMARCH=x86-64, or built on a host without FMA units: every f32 operation of the distance
     *        (Mm/GaussDiagonalMaximumFeatureScorer.cc:144-218) rounds once;
     *   fma  RASR's DEFAULT configuration (cmake_resources/CompileOptions.cmake:39-48: -march=native) built with GCC on an FMA host:
     *        `sum += df * df` is ONE fused multiply-add (vfmadd231ps / vfmadd231ss); about a fifth of the d = 40 distances differ in
     *        the last bit from the other build.  One vector operation fewer per dimension in the exact stage: the fused GMM kernel
     *        runs 4.60 -> 4.18 ms on BASELINE config 5's shard (profiles/r05/gmm_contract_ab.log) -- bench.py's default is fma because
     *        it is the reference's default build, and the line names the mode.
     *   Every mode takes both (round 6).  Bit-exact, in the named build: AMX_GMM_MAX scores and density indices, AMX_GMM_BATCH_FLOAT,
     *   AMX_GMM_PRESELECTION_FLOAT (clustering included), amx_gmm_best_density_dev, the quantised scorers (integer arithmetic; their
     *   host-side gaussLogNormFactor follows the contract).  AMX_GMM_SUM: the DISTANCES and the best density follow the contract bit
     *   for bit; the log-add score is the reference's two-pass form (the first minimum, then the sum of expf(best - s_k) in density order) on
     *   those bits with the device's expf / logf: not bit-exact (but bit-exact for one-density mixtures), within 1e-5 of the reference,
     *   and no further from the exact value of the same expression than 4x the reference's own f32 error plus 1e-6 max(1, |score|)
     *   on every kernel route (tests/test_gmm_sum_gpu.py).  Baum-Welch statistics: 2e-5 (the same expf).  fused_waves=13 (a lab kernel) has no fma
     *   form and fails the creation with AMX_ERR_UNSUPPORTED.  tests/test_gmm_contract_gpu.py, tests/test_contract_gpu.py.
     *
     * Kernel selection for A/B runs and tests -- every path gives the same scores and density indices bit for bit (within a contract):
     * screen=0 (no MFMA / f32 screen: every density evaluated), fused=0 (two-kernel screen path instead of gmm_fused_kernel),
     * screen_kernel=rows|persist|simple, graph=1 (HIP-graph replay of repeated small passes; off by default since round 6: plain launches
     * measured 3-5 % faster back to back and equal with a synchronisation per pass, profiles/r06/graph_ab.log), tied_prune=0|1 (tied models: dense tile
     * kernel | pruned scorer, default -1 adaptive), chunk=N (frames per internal pass, >= 256), fused_waves=8|12|16|13 (13: the
     * wave-specialised kernel), fr=2|4|8|16 (frames per workgroup of the uniform tied kernel), simd_mfma=0 (SIMD / batch-int scorers
     * without the i8 matrix kernel), dist_list=0 (pruned tied scorer: distances from the density-major kernel instead of the
     * list-order one; N >= 2: N frames per wave of the list-order kernel), near_fused=0 (the frame's near densities from
     * tied_near_kernel instead of the list-order kernel's atomic minima), fused_pack=0 (gmm_fused_kernel reads operand rows packed by
     * gmm_screen_pack_kernel instead of packing its own). */
    const char*     tuning;
} amx_gmm_model;

/* diagonal-maximum / diagonal-sum / batch-diagonal-maximum-float (Mm/BatchFeatureScorer.cc:164-254: pooled
 * covariance only, no best-density output, ignores the two scales like the reference class) /
 * SIMD-diagonal-maximum (Mm::SimdGaussDiagonalMaximumFeatureScorer, Mm/SimdFeatureScorer.cc:68-176 with
 * Mm/IntelOptimization.cc:37-66: means and features times scaling / sigma quantised to u8, integer distance and constant,
 * first minimum, score = 0.5 * min / scaling^2; assigns densities; ignores the two scales like the reference class) /
 * batch-diagonal-maximum-int and -fast (Mm::BatchIntFeatureScorer / BatchUnrolledIntFeatureScorer, Mm/BatchFeatureScorer.cc:375-504:
 * the same u8 quantisation and integer distance, pooled covariance only, constant (s32)(logNorm scale^2 - 2 scale^2 logWeight) formed
 * in f64, score = (f32)min / (2 scale^2) in f32, no best-density output) /
 * preselection-batch-float (see amx_gmm_set_preselection below; pooled covariance only, no best-density output) */
enum { AMX_GMM_MAX = 0, AMX_GMM_SUM = 1, AMX_GMM_BATCH_FLOAT = 2, AMX_GMM_SIMD = 3, AMX_GMM_BATCH_INT = 4, AMX_GMM_PRESELECTION_FLOAT = 5,
       AMX_GMM_PRESELECTION_INT = 6 };

int  amx_gmm_create(amx_ctx* ctx, const amx_gmm_model* model, amx_gmm** out); /* copies everything */
void amx_gmm_destroy(amx_gmm* h);
int  amx_gmm_n_mixtures(const amx_gmm* h);
int  amx_gmm_dimension(const amx_gmm* h);
/* the topology as amx_gmm_model holds it: *n_entries = mix_offsets[n_mix]; mix_offsets [n_mix + 1] and dens_index [n_entries] nullable */
int  amx_gmm_topology(const amx_gmm* h, int* n_entries, uint32_t* mix_offsets, uint32_t* dens_index);
/* host copies of the prepared scorer tables (Mm/MixtureFeatureScorerElement.cc:21-33,
 * Mm/CovarianceFeatureScorerElement.cc:21-51); any pointer may be NULL */
int amx_gmm_tables(const amx_gmm* h, float* minus2_log_weights, float* inv_sqrt_var, float* log_norm);
/* quantisation scaling factor of the SIMD-diagonal-maximum scorer (SimdGaussDiagonalMaximumFeatureScorer::getScaling,
 * logged as "Scaling factor"); 0 for a host-only handle */
float amx_gmm_simd_scaling(const amx_gmm* h);
/* preselection-batch-float (Mm::BatchPreselectionFloatFeatureScorer, Mm/BatchFeatureScorer.cc:256-318 with
 * Mm::FloatDensityClustering, Mm/DensityClustering.cc / .tcc): batch-diagonal-maximum-float restricted, per frame, to the densities
 * of the `select_clusters` clusters closest to the scaled feature; k-means over the pre-scaled density means (`clusters`
 * clusters, initial clusters drawn with srand(1) / rand(), `iterations` rounds); a mixture without an active density scores
 * `backoff_score`.  Defaults (the reference's): 256 / 32 / 5 / 40000.  The clustering is built on the first preselection call
 * (or amx_gmm_preselection_clustering) and rebuilt after amx_gmm_set_preselection.  amx_gmm_preselection_clustering returns
 * it: cluster_of [sum K_m] (cluster of every mixture entry), cluster_means [n_clusters x dim]; any pointer may be NULL.
 * Parity with the reference binary holds up to DISTANCE TIES between clusters: the reference ranks them with std::sort on the
 * distance alone (selectClusters), whose order among equal distances is implementation-defined; here (and in the oracle) the
 * lower cluster index wins.  Exact ties are rare in f32 and common in the u8 / s32 variant below -- there the selected cluster set,
 * and with it a score or a back-off value, can differ from a given reference build at a tie.  A frame whose distances are all NaN
 * selects the first `select_clusters` clusters (what an index-ordered sort of incomparable keys leaves in front). */
int amx_gmm_set_preselection(amx_gmm* h, int clusters, int select_clusters, int iterations, float backoff_score);
int amx_gmm_preselection_clustering(amx_gmm* h, int* n_clusters, uint32_t* cluster_of, float* cluster_means);
/* AMX_GMM_PRESELECTION_INT = Mm::BatchPreselectionIntFeatureScorer ("preselection-batch-int", Mm/BatchFeatureScorer.cc:514-578):
 * the batch-int scorer over the densities of the select-clusters clusters closest to the QUANTISED feature, with
 * Mm::DensityClustering<u8, s32> over the quantised means (integer distances, cluster means truncated to u8); a mixture without an
 * active density scores (f32)INT_MAX / scale_ -- the int class has no back-off score.  Same parameters
 * (amx_gmm_set_preselection; backoff_score unused).  cluster_means [n_clusters x dim]: the u8 values as floats. */
int amx_gmm_preselection_int_clustering(amx_gmm* h, int* n_clusters, uint32_t* cluster_of, float* cluster_means);
/* Diagnostics of the screened diagonal-maximum scorer (no reference counterpart; bench.py prints survivors per mixture):
 * returns and clears the number of densities evaluated exactly and the number of (frame, mixture) pairs scored since the
 * last call, and switches the counting on (enable != 0) or off for the following calls.  Synchronises the stream.  Zero for
 * models that do not take the fused screened path.  Tied models whose mixtures share one density list (pruned path,
 * gmm_tied.hip): survivors = (density, frame, 64-mixture tile) triples whose weight rows were read, pairs = triples submitted
 * (densities x frames x tiles); always counted. */
int amx_gmm_screen_counts(amx_gmm* h, int enable, unsigned long long* survivors, unsigned long long* pairs);
/* scores [T x n_mix]; best_density (nullable) [T x n_mix] = index within the mixture of the
 * minimising density (AssigningFeatureScorer::ScoreAndBestDensity). */
int amx_gmm_score(amx_gmm* h, int mode, const float* feats_host, int T, float* scores_host, uint32_t* best_density_host);
int amx_gmm_score_dev(amx_gmm* h, int mode, const float* feats_dev, int T, float* scores_dev, uint32_t* best_density_dev);
/* diagonal-maximum scores plus the per-epoch statistics of amx_stats_accumulate_dev for these frames (best state per
 * frame, per-state counts, sum of best scores), the counterpart of amx_ffnn_score_stats_dev.  For screened models the
 * arg-min over the states is taken inside the exact stage, so the [T x n_mix] score matrix is written once and not
 * re-read.  best_density_dev and best_state_dev are nullable. */
int amx_gmm_score_stats_dev(amx_gmm* h, const float* feats_dev, int T, float* scores_dev, uint32_t* best_density_dev,
                            uint32_t* best_state_dev, unsigned long long* state_counts_dev, double* score_sum_dev);
/* The same pass with the best densities as ONE BYTE per (frame, mixture): best_density_dev [T x n_mix] bytes, required, the same
 * index within the mixture (Mm::DensityInMixture, Mm/Types.hh:36, is u32 in RASR; no mixture of a real model comes near 255
 * densities), 0xff where the u32 form writes 0xffffffff.  A quarter of the u32 matrix's MEMORY -- for a 10 000-state model 10 kB
 * instead of 40 kB per frame, next to 40 kB of scores: 0.64 GB instead of 2.56 GB per 63 936-frame pass -- and no gain in TIME:
 * the fused screened kernel writes it directly, but what the best densities cost that kernel (0.3 ms of 4.7) is the vector work of
 * tracking them, not their bytes (tools/gmm_store_ab.py, profiles/r04/gmm_store_ab.log: 4.58-4.62 ms against 4.50-4.76 for u32,
 * 4.22-4.30 without).  Every other path scores into a u32 workspace and narrows it.
 * AMX_ERR_UNSUPPORTED for a model with a mixture of more than 255 densities. */
int amx_gmm_score_stats_u8_dev(amx_gmm* h, const float* feats_dev, int T, float* scores_dev, uint8_t* best_density_dev,
                               uint32_t* best_state_dev, unsigned long long* state_counts_dev, double* score_sum_dev);

/* Viterbi training statistics of Mm::AbstractMixtureSetEstimator::accumulate (Mm/AbstractMixtureSetEstimator.cc:117-125,
 * Mm/GaussDensityEstimator.hh:152-208): frame t, aligned to mixture_dev[t], adds 1 to the weight of its best density
 * (best_density_dev[t * best_density_ld + mixture] as written by amx_gmm_score_dev, or best_density_dev[t] when
 * best_density_ld == 0), x to that density's mean accumulator and x*x to its covariance accumulator, all in f64.
 * acc_dev is ONE flat f64 buffer -- [sum K_m weights][n_mean weights][n_mean x dim sums][n_cov weights][n_cov x dim sums],
 * amx_gmm_accumulator_size() doubles -- so that data-parallel ranks combine their statistics with a single all-reduce
 * (the reference combines per-partition accumulator files offline, Tools/AcousticModelTrainer/AcousticModelTrainer.cc:317-325). */
/* AssigningContextScorer::bestDensity(e) for ONE mixture per frame (Mm/AssigningFeatureScorer.hh:127-131 ->
 * GaussDiagonalMaximumFeatureScorer::calculateScoreAndDensity, Mm/GaussDiagonalMaximumFeatureScorer.cc:116-142): best_density_dev[t] =
 * index within mixture_dev[t] of the density that minimises frame t's score, scores_dev[t] (nullable) that score -- the same bits as
 * entry (t, mixture_dev[t]) of amx_gmm_score_dev's matrices (0xffffffff / Type<f32>::max for a mixture index >= n_mix).  It is what the
 * Viterbi accumulation asks of an assigning scorer: a trainer that scores every state (amx_gmm_score_stats_dev with
 * best_density_dev = NULL: the screened kernel is 0.3 ms of 4.7 faster without the index bookkeeping) needs the density of the
 * ALIGNED state only, and gets it here for amx_gmm_accumulate_dev(..., best_density_ld = 0). */
int amx_gmm_best_density_dev(amx_gmm* h, const float* feats_dev, int T, const uint32_t* mixture_dev, uint32_t* best_density_dev,
                             float* scores_dev);
long amx_gmm_accumulator_size(const amx_gmm* h);
int  amx_gmm_accumulate_dev(amx_gmm* h, const float* feats_dev, int T, const uint32_t* mixture_dev,
                            const uint32_t* best_density_dev, int best_density_ld, double* acc_dev);
/* the same statistics from the byte form of the best-density matrix (amx_gmm_score_stats_u8_dev) */
int  amx_gmm_accumulate_u8_dev(amx_gmm* h, const float* feats_dev, int T, const uint32_t* mixture_dev,
                               const uint8_t* best_density_dev, int best_density_ld, double* acc_dev);

/* The same statistics as a binary "MIXSET" accumulator file, version 2 (Mm::MixtureSetEstimator::write / read,
 * src/Mm/AbstractMixtureSetEstimator.cc:404-508, src/Mm/VectorAccumulator.hh:80-100, src/Mm/MixtureEstimator.cc:140-170):
 * what RASR's accumulate / combine-mixture-set-estimators / estimate actions exchange.  acc_host is the flat buffer of
 * amx_gmm_accumulator_size() doubles (host memory); read requires the file's topology to equal the model's. */
int amx_gmm_accumulator_write(const amx_gmm* h, const double* acc_host, const char* path);
int amx_gmm_accumulator_read(const amx_gmm* h, const char* path, double* acc_host);

/* Weighted Viterbi / Baum-Welch statistics: Mm::AbstractMixtureSetEstimator::accumulate(mixture, x, weight)
 * (Mm/AbstractMixtureSetEstimator.cc:127-147).  weight_dev: per-frame f64 weights (the alignment's posterior weight), NULL = 1.
 *   AMX_GMM_VITERBI     the best density (best_density_dev as above) gets the whole frame weight;
 *   AMX_GMM_BAUM_WELCH  every density k of the aligned mixture gets weight * exp(score(e) - s_k), the density posterior of
 *                       the log-add scorer (Mm/GaussDiagonalMaximumFeatureScorer.cc:291-298), if that product exceeds
 *                       Core::Type<f32>::epsilon; best_density_dev is not used.
 * Sums are weight * x and (weight * x) * x in f64 (plusWeighted / plusSquareWeighted, Mm/Utilities.hh:108-153). */
enum { AMX_GMM_VITERBI = 0, AMX_GMM_BAUM_WELCH = 1 };
int amx_gmm_accumulate_weighted_dev(amx_gmm* h, int mode, const float* feats_dev, int T, const uint32_t* mixture_dev,
                                    const double* weight_dev, const uint32_t* best_density_dev, int best_density_ld,
                                    double* acc_dev);

/* Re-estimation from the (all-reduced) statistics: Mm::AbstractMixtureSetEstimator::estimate
 * (Mm/AbstractMixtureSetEstimator.cc:305-338: densities below the observation-weight limits leave their mixture except
 * the heaviest one, Mm/MixtureEstimator.cc:64-82; remaining densities / means / covariances are renumbered in order of
 * first appearance, :804-817; mixture weights log(w) normalised by logExpNorm, Mm/Mixture.cc:63-74; mean = sum / weight,
 * variance = (sum x^2 - sum_j sum_j^2 / N_j) / N floored at min_variance, Mm/GaussDensityEstimator.cc:148-233), and with
 * cfg->split the acoustic model trainer's splitting step on top of it (Mm::MixtureSetSplitter::split,
 * Mm/MixtureSetSplitter.cc:38-123: means with enough observations become mean +- sqrt(var) * perturbation * f32 epsilon).
 * `topology` is the model the statistics were accumulated with (its means / variances / weights are not read); acc_host the
 * flat buffer of amx_gmm_accumulator_size() doubles.  The result is a mixture set like amx_pms_read's: view it, write it
 * with amx_pms_write, or build the next iteration's scorer from it.  Host work, model-sized, once per epoch. */
typedef struct {
    double min_observation_weight;    /* minimum-observation-weight, default 5 */
    double min_relative_weight;       /* minimum-relative-weight, default 0 */
    double min_variance;              /* minimum-variance, default 0 (compared and stored as f32) */
    int    normalize_mixture_weights; /* normalize-mixture-weights, default 1 */
    int    allow_zero_weights;        /* allow-zero-weights, default 0: a mixture without observations is an error */
    int    split;                     /* 0: estimate only; 1: estimate, then split */
    double split_min_mean_observation_weight;       /* minimum-mean-observation-weight, default 20 */
    double split_min_covariance_observation_weight; /* minimum-covariance-observation-weight, default f32 max (never) */
    double split_perturbation_weight;               /* perturbation-weight, default 0.1 */
    int    split_normalize_mixture_weights;         /* normalize-mixture-weights of the splitter, default 0 */
} amx_gmm_estimate_cfg;
typedef struct amx_mixture_set amx_mixture_set;
void amx_gmm_estimate_cfg_default(amx_gmm_estimate_cfg* cfg);
int  amx_gmm_estimate(const amx_gmm_model* topology, const double* acc_host, const amx_gmm_estimate_cfg* cfg /* NULL: defaults */,
                      amx_mixture_set** out);

/* ------------------------------------------------------------------ LDA estimation: scatter matrices */

/* Signal::ScatterMatricesEstimator (src/Signal/ScatterEstimator.cc), the corpus pass behind the matrix that amx_matrix_multiply_dev
 * applies: Speech::TextDependentScatterMatricesEstimator::processAlignedFeature hands it every aligned frame with the emission
 * index of the alignment as its class.  The accumulator is ONE flat f64 buffer,
 *   [dim (dim + 1) / 2 square sums, lower triangle, row-major] [n_classes x dim class vector sums] [n_classes class counts]
 * -- amx_scatter_accumulator_size() doubles, 0 for a shape outside 1 <= dim <= 1024, n_classes >= 1 -- which is the order of the
 * accumulator file behind its two u32 headers (ScatterEstimator.cc:95-106, 359-376), so that data-parallel ranks combine with the one
 * amx_comm_all_reduce_f64_dev they already issue (the reference: `combine-scatter-matrix-accus`, ScatterEstimator.cc:407-417). */
long amx_scatter_accumulator_size(int dim, int n_classes);
/* ScatterMatricesEstimator::accumulate(classIndex, x, weight) (ScatterEstimator.cc:227-234 -> :44-55) for T frames
 * feats_dev[t * in_ld + 0 .. dim) of class class_dev[t] and f32 weight weight_dev[t] (NULL: 1), ADDED into acc_dev:
 *   square[i][j] += (f64)((x_i * x_j) * w) for j <= i   both products in f32, in that order, then widened
 *   sums[c][i]   += (f64)(x_i * w)                      x * weight is a Math::Vector<f32>
 *   counts[c]    += (f64)w
 * Nothing here can be contracted, so both amx_set_contract settings give the same bits.  A frame whose class is >= n_classes
 * (0xffffffff: no label) is skipped; a NaN reaches the sums it touches.  in_ld >= dim; sums across workgroups are f64 atomics
 * (order undefined; exact where no addition rounds).  AMX_ERR_INVALID with a named amx_last_error for a bad argument. */
int amx_scatter_accumulate_dev(amx_ctx* ctx, const float* feats_dev, int in_ld, long T, int dim, const uint32_t* class_dev, int n_classes,
                               const float* weight_dev /* NULL: 1 */, double* acc_dev);
/* The accumulator file of ScatterMatricesEstimator::write / read (ScatterEstimator.cc:79-106, 337-376; `new-accumulator-file`,
 * `old-accumulator-file`, `accumulator-files-to-combine`): u32 dim, the triangle, u32 nClasses, sums, counts; little endian.
 * acc_host is the flat buffer in host memory; read allocates it (release with amx_free). */
int amx_scatter_accumulator_write(int dim, int n_classes, const double* acc_host, const char* path);
int amx_scatter_accumulator_read(const char* path, int* dim, int* n_classes, double** acc_host /* amx_free */);
/* ScatterMatricesEstimator::finalize (ScatterEstimator.cc:245-285, 72-77, 287-292; hh:141-143), host, f64, the reference's order of
 * operations: total-mean part (s_i s_j) / N, class-mean part sum over classes with n_c > 0 of (s_ci s_cj) / n_c,
 * between = class-mean - total-mean, within = square - class-mean, total = square - total-mean, each times 1 / N when normalize
 * (`shall-normalize`); the square sum's upper triangle mirrors its lower.  N = 0: AMX_ERR_INVALID ("No observation has been seen.").
 * The eigenvalue step (Signal::LinearDiscriminantAnalysis) stays with RASR: write the matrices with amx_matrix_write_f64. */
int amx_scatter_finalize(int dim, int n_classes, const double* acc_host, int normalize, double* between, double* within,
                         double* total /* each dim x dim row-major, nullable */);
/* Binary Math::Matrix<f64> (Math/Matrix.hh:560-574; Math/Module.cc:35 registers "bin" for Matrix<f64>): the f64 twins of
 * amx_nn_matrix_read / amx_nn_matrix_write, same layout, an optional "bin:" prefix.  *data is malloc'ed; release it with amx_free. */
int amx_matrix_read_f64(const char* path, int* rows, int* cols, double** data);
int amx_matrix_write_f64(const char* path, int rows, int cols, const double* data);

/* ------------------------------------------------------------------ histogram normalisation (per-speaker): estimation, files, apply */

/* amx_histogram is one Signal::HistogramVector<f32> (Signal/Histogram.hh:85-103): `dim` histograms of one bucket size (the estimator's
 * `bucket-size`, 0.0002 by default, Speech/HistogramEstimator.cc:19-20), each a LookupTable that grows (Signal/LookupTable.hh:50-66).
 * State after any number of calls, per dimension: offset = -min k, size = max k - min k + 1 over everything accumulated, where
 * k = (s32)round(x / bucket_size) (LookupTable.hh:69-72: f32 division, round half away from zero), grow = true, value[b] = number of
 * frames in bucket b as f32.  The reference adds 1.0f in f32 (Histogram.hh:46-48), so a value stops at 16 777 216; the handle counts in
 * u32 and exports (float)min(count, 2^24).  A handle takes at most 2^32 - 1 frames; a call that would pass that is refused.
 * A frame holding a NaN, an infinity or a value with |x / bucket_size| >= 2^30 makes accumulate return AMX_ERR_INVALID and add NOTHING
 * of that call: the reference's cast to s32 is undefined there.  Weights are not taken (the estimator passes 1, HistogramEstimator.cc).
 * A call holds the frames of ONE corpus key.  ctx may be NULL: a host-only handle for files and tables (amx_histogram_attach gives it a
 * context later).  Nothing here depends on amx_set_contract: no multiply of this arithmetic feeds an add. */
typedef struct amx_histogram amx_histogram;
typedef struct {
    int   dim;
    float bucket_size;
    int   frozen;          /* read from a file whose values are not counts: serves tables, refuses accumulate */
    int   lds_max_buckets; /* a dimension whose window has at most this many buckets counts in a workgroup-private LDS table ... */
    int   lds_capacity;    /* ... while the windows of such dimensions, taken in order, fit this many buckets in all; the rest use memory atomics */
    unsigned long long frames;         /* accumulated so far (after a file: the largest sum of one dimension) */
    unsigned long long n_lds;          /* (dimension, device call) pairs that counted in LDS */
    unsigned long long n_global;       /* ... that counted with atomics on memory */
    unsigned long long n_device_calls; /* amx_histogram_accumulate_dev calls that added frames; each synchronises the stream once */
} amx_histogram_info;
int  amx_histogram_create(amx_ctx* ctx /* nullable */, int dim /* 1 .. 4096 */, float bucket_size /* > 0 */, amx_histogram** out);
void amx_histogram_destroy(amx_histogram* h);
int  amx_histogram_attach(amx_histogram* h, amx_ctx* ctx);
int  amx_histogram_describe(const amx_histogram* h, amx_histogram_info* info);
/* HistogramVector::accumulate (Histogram.hh:107-112) for T frames feats_dev[t * in_ld + 0 .. dim).  Synchronises the context's stream
 * once (the range of the call's buckets comes back to the host, which grows the tables).  Calls in any split give the same tables. */
int  amx_histogram_accumulate_dev(amx_histogram* h, const float* feats_dev, int in_ld, long T);
/* The same on the host, in plain C++ (a handle without a context; small corrections to a histogram read from a file). */
int  amx_histogram_accumulate(amx_histogram* h, const float* feats_host, int in_ld, long T);
/* HistogramVector::write / read (Histogram.hh:122-135; LookupTable::write / read, LookupTable.hh:298-319; Core::BinaryOutputStream, little
 * endian): u32 n | n x (f32 bucketSize, s32 offset, one byte grow (0xff = true, Core/BinaryStream.cc:95-103), u32 size, f32 values[size]).  This is the per-key file of the
 * estimator's object cache (Core/ObjectCache.hh:488-517) and the training-histogram file of the normalisation node.  A file whose values
 * are all whole numbers <= 2^24 in growing tables of one bucket size resumes counting; any other file loads frozen. */
int  amx_histogram_write(const amx_histogram* h, const char* path);
int  amx_histogram_read(const char* path, amx_histogram** out);
/* One dimension: the table itself, Histogram::getCdf (Histogram.hh:73-80: sequential f32 partial sums divided by the sequential f32 sum;
 * an empty histogram is AMX_ERR_INVALID), Histogram::percentile (Histogram.hh:56-64).  values nullable: ask for *size first. */
int  amx_histogram_table(const amx_histogram* h, int d, float* bucket_size, int* offset, int* size, float* values);
int  amx_histogram_cdf(const amx_histogram* h, int d, float* bucket_size, int* offset, int* size, float* values);
int  amx_histogram_percentile(const amx_histogram* h, int d, float percent, float* value);

/* amx_histnorm is Signal::HistogramNormalization (Signal/HistogramNormalization.hh:26-68): inverse CDFs of the training histograms, test
 * CDFs per corpus key, out[i] = inverse_i[ cdf_i[ in[i] ] ] (HistogramNormalization.cc:68-75).
 * One training histogram: setTrainingHistograms(histograms, bucketSize) (HistogramNormalization.cc:24-34).  Several: the interpolated form
 * (:36-60) -- normalizeSurface, *= scale, += into tables of the minimal bucket size -- built by amx_histnorm_set_scales from the
 * n_train - 1 scales of the node's scale ports; the first scale is 1 - their sum (normalizeScales, :91-93) and a scale outside [0, 1] is
 * AMX_ERR_INVALID (areScalesWellDefined, :77-84).  Until then such a handle cannot apply (AMX_ERR_STATE).  probability_bucket_size = 0
 * selects LookupTable::proposeBucketSizeForInverse (LookupTable.hh:264-271); the inverse follows LookupTable::getInverse (:239-262).
 * The training histograms are copied: they may be destroyed afterwards.  ctx may be NULL (tables only). */
typedef struct amx_histnorm amx_histnorm;
int  amx_histnorm_create(amx_ctx* ctx /* nullable */, int n_train, const amx_histogram* const* train, float probability_bucket_size, amx_histnorm** out);
void amx_histnorm_destroy(amx_histnorm* h);
int  amx_histnorm_set_scales(amx_histnorm* h, const float* scales /* [n_train - 1] */);
/* setTestHistograms (HistogramNormalization.cc:62-66) for one more corpus key; *key is its number in amx_histnorm_apply_dev.  A histogram
 * of another dimension is AMX_ERR_INVALID (HistogramNormalizationNode::init, :176-181), an empty one too. */
int  amx_histnorm_add_key(amx_histnorm* h, const amx_histogram* test, int* key);
int  amx_histnorm_n_keys(const amx_histnorm* h);
int  amx_histnorm_inverse_cdf(const amx_histnorm* h, int d, float* bucket_size, int* offset, int* size, float* values /* nullable */);
int  amx_histnorm_test_cdf(const amx_histnorm* h, int key, int d, float* bucket_size, int* offset, int* size, float* values /* nullable */);
/* apply() on frames [frame_offsets[0], frame_offsets[n_seg]) of in_dev, one launch; segment s = frames [frame_offsets[s],
 * frame_offsets[s + 1]) uses key key_of_segment[s] (both lists on the host).  in_dev == out_dev is allowed; columns >= dim are not touched.
 * Per element: b = (s32)round(x / bs_test) + off_test, p = cdf[b], b2 = (s32)round(p / bs_inv) + off_inv, out = inverse[b2]
 * (LookupTable.hh:69-72, 108-112).  A bucket outside its table is undefined in the reference's release build (the `ensure_` of :110 is
 * compiled out); here it is the nearest end bucket, which is what LookupTable::insert does on a table that may not grow (:178-202).
 * clamped (nullable, host): [0] = elements clamped at the test CDF, [1] = at the inverse; asking for it synchronises the stream.
 * A NaN input gives a NaN output and counts in clamped[0]. */
int  amx_histnorm_apply_dev(amx_histnorm* h, int n_seg, const long* frame_offsets, const int* key_of_segment, const float* in_dev, int in_ld,
                            float* out_dev, int out_ld, unsigned long long clamped[2]);

/* ------------------------------------------------------------------ Bayes classification: segment, continuous and windowed decisions */

/* amx_bayes is one Signal::BayesClassification (Signal/BayesClassification.hh:36-151) with the uniform prior and the independent-sequence
 * likelihood, the only types the reference has: the arithmetic of the nodes `signal-bayes-classification` and
 * `signal-bayes-classification-score` (Signal/Module.cc:126-129) on a [frames x classes] score matrix that a scorer left on the device.
 * All values are f32.  Per frame t and class c: s = w_t * score(t, c), rounded once (LikelihoodFunction.cc:77); scores_[c] += s in frame
 * order (:80); sumOfWeights += w_t (LikelihoodFunction.hh:55); w_t = 1 without a weight stream.  Both builds of the reference compute
 * this alike (the product is stored as well as added, so it is not contracted): nothing here depends on amx_set_contract.
 * Prior: logN = std::log((f32)n_classes) (AprioriProbability.cc:20).  Decision (argMin, BayesClassification.cc:135-161): per class
 * score = logN, then += scores_[c] without a window, or += every stored s of the window FROM THE NEWEST FRAME TO THE OLDEST with one; strict
 * `<` from FLT_MAX picks the label, so the first minimum wins and a NaN or a value >= FLT_MAX never does.  Where no class wins the
 * reference indexes out of range; here the label is -1 and a counter reports it.
 * Modes (classify, work: :103-119, :384-411):
 *   segment     number_of_features, delay, window_length unset: one label at the end of the stream over all frames; none for 0 frames.
 *   first N     number_of_features = N: the label after frame N - 1 over frames 0 .. N - 1, later frames are not scored; N >= T: segment mode.
 *   continuous  delay = d: a label after every frame t >= d over frames 0 .. t; when no frame reached t >= d, one label at the end of
 *               the stream.
 *   windowed    window_length = L: the window holds the last L frames; a label after every frame once it is full (delay unset), or when it
 *               is full and at least d frames came since the last label; one more label at the end of the stream, over what the window
 *               holds, if frames came after the last label or the window never filled.  window_right does not change what the window
 *               holds (SlidingWindow.hh:445-452) but must be < L.
 * Refused with AMX_ERR_INVALID, the message naming the parameter: n_classes < 1; window_right >= window_length (the reference's init fails);
 * a window together with number_of_features, and delay together with number_of_features (the reference lets both through and emits a
 * label at frame N - 1 that belongs to neither mode). */
typedef struct {
    int  n_classes;            /* >= 1 */
    long number_of_features;   /* <= 0 or >= INT_MAX: all frames */
    long delay;                /* < 0 or >= INT_MAX: no continuous output */
    int  window_length;        /* <= 0: no window */
    int  window_right;         /* must be < window_length when a window is used */
    int  single_frame;         /* score node only: single-frame-classification */
} amx_bayes_cfg;
typedef struct amx_bayes amx_bayes;
void amx_bayes_default_cfg(amx_bayes_cfg* cfg); /* the node's defaults (:294-303): segment mode; n_classes 0 has to be set */
int  amx_bayes_create(amx_ctx* ctx /* nullable: configuration and prior only */, const amx_bayes_cfg* cfg, amx_bayes** out);
void amx_bayes_destroy(amx_bayes* h);
int  amx_bayes_prior(const amx_bayes* h, float* log_n_classes); /* UniformAprioriProbability::setClasses (AprioriProbability.cc:19-22) */
/* BayesClassificationNode::work (:384-411) for n_seg segments in one launch sequence.  Segment s = frames [frame_offsets[s],
 * frame_offsets[s + 1]) (host list, absolute row numbers) of scores_dev[t * scores_ld + c], weights_dev[t] (NULL: 1) and frame_label_dev[t].
 *   segment_label_dev[s]  the label that leaves at the end of the stream, or the single label of segment / first-N mode; -1 where the
 *                         reference emits none (no frames; continuous or windowed mode whose last frame emitted its own label)
 *   segment_score_dev     nullable, [n_seg x n_classes]: logN + sum per class as argMin formed it for that label; rows of segments
 *                         without such a label keep what the buffer held
 *   frame_label_dev[t]    continuous and windowed mode (required there, ignored otherwise): the label emitted after frame t, -1 where none is
 *   sum_of_weights_dev    nullable, [n_seg]: sumOfWeights() at the end of the stream (first-N mode: over the frames scored)
 *   no_winner             nullable, host: [0] = segment labels, [1] = frame labels that are -1 because no class won; asking synchronises
 * A weight of a scored frame that is negative or NaN (BayesClassificationNode::featureScoreWeight, :364-382, a critical error there) fails
 * the call with AMX_ERR_INVALID naming the first such frame, and nothing is written; with weights the call synchronises the stream once.
 * The call keeps frames x n_classes floats of scratch in the handle in continuous and windowed mode. */
int  amx_bayes_classify_dev(amx_bayes* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const float* scores_dev, int scores_ld,
                            const float* weights_dev, int32_t* segment_label_dev, float* segment_score_dev, int32_t* frame_label_dev,
                            float* sum_of_weights_dev, unsigned long long no_winner[2]);
/* BayesClassificationScoreNode::work (:429-444; getScores :121-133, :182-189): after every frame t >= delay the vector logN + scores_[c]
 * of the cumulative sums (never the window) leaves; with single_frame the sums are reset after each vector, so a vector leaves every
 * delay + 1 frames over those frames.  Row t of out_dev[t * out_ld + c] is written where a vector leaves after frame t (emitted_dev[t] = 1).
 * The vector that leaves at the end of the stream, when frames came after the last one, is stored in the row of the segment's last frame
 * (emitted_dev[t] = 2).  Other rows keep what the buffer held (emitted_dev[t] = 0).  number_of_features and the window do not act here. */
int  amx_bayes_scores_dev(amx_bayes* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const float* scores_dev, int scores_ld,
                          const float* weights_dev, float* out_dev, int out_ld, uint8_t* emitted_dev);
/* The fast-VTLN composition (one mixture per warping factor): amx_gmm_score_dev(gmm, mode, feats_dev + frame_offsets[0] * dim, frames)
 * into a score matrix the handle owns, then amx_bayes_classify_dev on it.  feats_dev is [frames x amx_gmm_dimension(gmm)], dense.
 * amx_gmm_n_mixtures(gmm) != n_classes is AMX_ERR_INVALID (IndependentSequenceLikelihood::setClasses, LikelihoodFunction.cc:34-45). */
int  amx_bayes_classify_gmm_dev(amx_bayes* h, amx_gmm* gmm, int mode, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const float* feats_dev,
                                const float* weights_dev, int32_t* segment_label_dev, float* segment_score_dev, int32_t* frame_label_dev,
                                float* sum_of_weights_dev, unsigned long long no_winner[2]);

/* ------------------------------------------------------------------ State posteriors: p(mixture | x) from a score matrix on the device */

/* amx_posterior is one Mm::StatePosteriorFeatureScorer (Mm/StatePosteriorFeatureScorer.{hh,cc}) with viterbi = true, working on
 * scores_dev[t * scores_ld + m] (f32, as any scorer of this library leaves it) for T frames.  All arithmetic is f64 (Mm::Weight,
 * Mm/Types.hh:30) with the device's double exp and log1p.  Per frame, over the mixtures m of the filter, in this order:
 *   s(m)      = prior(m) + scale * score(t, m)                                                   (cc:43, cc:90, cc:265)
 *   min, imin = the smallest s below DBL_MAX and its mixture; strict <, the FIRST index wins     (cc:49-52; the reference's choice
 *               among equal values follows its hash order and changes no value)
 *   stored(m) = s(m), in density-keyed mode + margin where m == margin_mixture[t]                (cc:45-48: the minimum is taken over
 *               the un-margined values)
 *   survivors = every m of the filter when pruning_threshold == DBL_MAX, else stored(m) < pruning_threshold + min   (cc:105-116)
 *   p(m)      = min - stored(m)                                                                  (cc:134)
 *   sum       = sum of exp(p(m)) over the survivors except imin's own entry                      (cc:135-137)
 *   logZs     = log1p(sum); posterior(m) = exp(p(m) - logZs); logZ = logZs - min                 (cc:139-143)
 * Mixture likelihoods (workMixtureLikelihoods, cc:162-165, 201-207): exp(-stored(m)) per survivor; log_z_dev is not written.
 * s follows amx_set_contract: the reference's -march=native build contracts it into one fused multiply-add
 * (tests/golden/ref_posterior.npz records where the two builds differ: wherever scale != 1 and the prior is not 0).
 * The order of the f64 sum is fixed per row (the reference's is the iteration order of a std::unordered_map): a frame's results are
 * the same bits whatever the batch, the frame's place in it or the other frames.  Against the reference logZ and the f64 posteriors
 * agree to 1e-11 relative (a reordered sum of n <= 16384 non-negative terms moves by (n - 1) * 2^-53).
 * Deviation, on purpose: in the reference the MIXTURE paths never assign minimumScore_ (workMixtureScores, cc:81-102, leaves it at the
 * DBL_MAX of reset()), so posteriorsAndMixtures() there yields 0 everywhere with logZ = inf and pruneScores prunes nothing.  Here the
 * mixture modes compute the lines above, which is what the reference's density path computes for one density per mixture.
 * Filter (a prior per mixture): the default is every mixture with prior 0 (DefaultFilter, cc:361-368).  The disregard list is erased
 * from the filter AS MIXTURE INDICES, whatever the parameter's name says (hh:148-154: filter_->erase(*it) on a map keyed by mixture);
 * numbers that name no mixture of the filter do nothing.
 * Refused: viterbi = 0 with AMX_ERR_UNSUPPORTED naming `viterbi` (it needs per-density scores no scorer here exports); n_mixtures < 1,
 * a filter index out of range, a filter that is empty (also once the disregard list is erased) with AMX_ERR_INVALID.  Context
 * priors, the statistics channel and Mc::ScaleUpdate have no counterpart.
 * Added rules: a frame in which no mixture of the filter has s < DBL_MAX, or whose minimum is -inf, gets min index -1, min DBL_MAX,
 * logZ 0, outputs 0 and no survivors, and is counted (no_minimum, host, nullable; asking synchronises the stream). */
typedef struct {
    int    n_mixtures;         /* >= 1 */
    double scale;              /* 1 */
    double pruning_threshold;  /* DBL_MAX: none */
    double margin;             /* 0; acts in density-keyed mode */
    int    viterbi;            /* 1; 0 is refused */
} amx_posterior_cfg;
enum { AMX_POSTERIOR_MIXTURE = 0 /* workMixturePosteriors */, AMX_POSTERIOR_LIKELIHOOD = 1 /* workMixtureLikelihoods */,
       AMX_POSTERIOR_DENSITY = 2 /* workDensityPosteriors */ };
/* Outputs of one call, each nullable (the three sparse arrays together).
 *   posterior_f32_dev / posterior_f64_dev  [T x ld], ld >= n_mixtures: column m holds mixture m's value, 0 where m was filtered or pruned;
 *                                          the f32 value is the narrowed f64 one (the Flow node's Sparse::Vector<f32>)
 *   log_z_dev, min_dev [T] f64; min_index_dev [T]: imin (a MIXTURE index in every mode); n_survivors_dev [T]
 *   sparse_index_dev / sparse_value_dev    [T x sparse_capacity]: the survivors' (index, f32 value) in increasing mixture order;
 *   sparse_count_dev [T]                   the number of survivors.  A frame with more survivors than sparse_capacity keeps the first
 *                                          sparse_capacity of them; nothing is written outside its row, entries past the count keep
 *                                          what they held.  In density-keyed mode index = topology[m][best_density(t, m)]. */
typedef struct {
    float*   posterior_f32_dev;
    int      posterior_f32_ld;
    double*  posterior_f64_dev;
    int      posterior_f64_ld;
    double*  log_z_dev;
    double*  min_dev;
    int32_t* min_index_dev;
    int32_t* n_survivors_dev;
    int32_t* sparse_index_dev;
    float*   sparse_value_dev;
    int32_t* sparse_count_dev;
    int      sparse_capacity;
} amx_posterior_out;
typedef struct amx_posterior amx_posterior;
void amx_posterior_default_cfg(amx_posterior_cfg* cfg); /* the parameters' defaults (cc:289-313); n_mixtures 0 has to be set */
int  amx_posterior_create(amx_ctx* ctx /* nullable: configuration only */, const amx_posterior_cfg* cfg, amx_posterior** out);
void amx_posterior_destroy(amx_posterior* h);
/* the filter: n (mixture, prior) pairs (prior NULL: 0); a repeated mixture keeps its last prior.  On failure the old filter stays. */
int  amx_posterior_set_filter(amx_posterior* h, int n, const int* mixture, const double* prior);
int  amx_posterior_set_default_filter(amx_posterior* h);             /* setDefaultFilter (hh:220-222) */
int  amx_posterior_set_single_filter(amx_posterior* h, int mixture); /* setFilter(mixtureIndex) (cc:401-403) */
int  amx_posterior_set_disregard(amx_posterior* h, int n, const int* numbers); /* paramDisregardDensities; applies to every filter set */
/* the filter in effect (without the disregarded mixtures), in increasing mixture order; mixture and prior nullable, [n_mixtures] */
int  amx_posterior_filter(const amx_posterior* h, int* n, int* mixture, double* prior);
/* Density-keyed mode: topology[m] = dens_index[mix_offsets[m] .. mix_offsets[m + 1]) (the fields of amx_gmm_model), or taken from a
 * GMM scorer.  monotone: every density number of mixture m is below those of mixture m + 1, so the sparse form's mixture order is
 * also increasing key order (otherwise the adapter sorts each row, as StatePosteriorFeatureScorerNode.cc:49-57 does).
 * shared_density: a density that two mixtures list (-1: none).  With one the reference's map keeps whichever mixture its hash order
 * visits last; density-keyed calls are refused with AMX_ERR_UNSUPPORTED naming the density. */
int  amx_posterior_set_topology(amx_posterior* h, const uint32_t* mix_offsets /*[n_mixtures+1]*/, const uint32_t* dens_index);
int  amx_posterior_set_topology_gmm(amx_posterior* h, const amx_gmm* gmm);
int  amx_posterior_topology_info(const amx_posterior* h, int* monotone, long long* shared_density);
/* One launch on the context's stream.  mode AMX_POSTERIOR_DENSITY needs best_density_dev[t * best_ld + m] (u32, the matrix
 * amx_gmm_score_dev writes; a value past the mixture's list is read as its last density) and takes margin_mixture_dev[t]
 * (nullable; -1: none), which the other modes refuse.  The dense outputs stay keyed by mixture in every mode. */
int  amx_posterior_dev(amx_posterior* h, int mode, const float* scores_dev, int scores_ld, int T, const uint32_t* best_density_dev, int best_ld,
                       const int32_t* margin_mixture_dev, const amx_posterior_out* out, unsigned long long* no_minimum);
/* posteriorsAndMixtures(IndicesAndWeights&) (cc:258-284): frame t has the candidates [list_offsets[t], list_offsets[t + 1]) (host list) of
 * mixture_dev[i] / prior_dev[i]; s, the minimum (first in LIST order), sum, log1p and the posteriors as above over the list only, no
 * filter, no pruning, no margin; one posterior per entry into posterior_f64_dev[i] and/or posterior_f32_dev[i].  A mixture outside
 * [0, n_mixtures) is never read: its score is +inf.  A list without a minimum gets posteriors 0 and is counted.
 * The call synchronises the stream once (the host list is copied and waited for). */
int  amx_posterior_lists_dev(amx_posterior* h, const float* scores_dev, int scores_ld, int T, const long long* list_offsets /*[T+1]*/,
                             const int32_t* mixture_dev, const double* prior_dev, double* posterior_f64_dev, float* posterior_f32_dev,
                             unsigned long long* no_minimum);
/* amx_gmm_score_dev(gmm, gmm_mode, feats_dev, T) into a score matrix (and, in density-keyed mode, a best-density matrix) the handle
 * owns, then amx_posterior_dev on it.  feats_dev is [T x amx_gmm_dimension(gmm)], dense. */
int  amx_posterior_gmm_dev(amx_posterior* h, amx_gmm* gmm, int gmm_mode, int mode, const float* feats_dev, int T, const int32_t* margin_mixture_dev,
                           const amx_posterior_out* out, unsigned long long* no_minimum);

/* ------------------------------------------------------------------ Model combination: log-linear sum of several score matrices */

/* amx_combine is one Mm::CombinedFeatureScorer: out[t][e] = ((0 + r_0) + r_1) + ... in model order (CombinedFeatureScorer.cc:42-59),
 * r_i = scale_i * scores_i[t][table[e][i]] (ScaledContextScorer::score, ScaledFeatureScorer.hh:65-67), all f32, every product rounded
 * before it is added (it is a virtual call's return value; both builds of the reference agree, so nothing follows amx_set_contract).
 * table is [n_emissions x n_models]; an entry outside [0, n_mixtures[i]) is AMX_ERR_INVALID (verifyMixtureIndexTable, :85-100), as
 * are n_models outside 1 .. AMX_COMBINE_MAX_MODELS and n_emissions < 1.  A column that is 0, 1, 2, ... is read straight, any other
 * through the table.  out_dev may overlap none of the inputs (AMX_ERR_INVALID). */
#define AMX_COMBINE_MAX_MODELS 8
typedef struct amx_combine amx_combine;
int  amx_combine_create(amx_ctx* ctx /* nullable: validation only */, int n_models, int n_emissions, const int* n_mixtures /*[n_models]*/,
                        const int* table, const float* scale /*[n_models]*/, amx_combine** out);
void amx_combine_destroy(amx_combine* h);
int  amx_combine_identity_columns(const amx_combine* h, unsigned* mask); /* bit i: column i is read straight */
int  amx_combine_dev(amx_combine* h, int T, const float* const* scores_dev /*[n_models]*/, const int* ld /*[n_models]*/, float* out_dev, int out_ld);

/* ------------------------------------------------------------------ Viterbi alignment on the score matrix: search, traceback, labels */

/* amx_align is one Search::Aligner in Viterbi mode (Search/Aligner.cc:41-470, 530-651; what Speech::AlignmentNode runs): the
 * time-synchronous search over an epsilon-free acceptor whose arcs consume one frame each, on scores_dev[t * scores_ld + e] (f32, as any
 * scorer of this library leaves it).  Only f32 additions and comparisons: nothing here depends on amx_set_contract.
 *   expansion      per frame, per hypothesis in list order, per arc in arc order: sco = (score + weight) + emission (:234);
 *                  emission = score_scale * scores[t][e], rounded once when score_scale != 1 (ScaledContextScorer::score)
 *   recombination  the first candidate of a target creates its hypothesis and fixes its place in the frame's list; a later one replaces
 *                  score, trace and label when old >= new (:144-167): the LAST of the candidates with the minimal score wins
 *   pruning        survivors have score <= minimumScore() + threshold, order kept (:254-318, :594-601)
 *   iteration      for (t = min; t <= max; t *= factor), restarting per pass (:603-630); a pass ends the loop when a final state is
 *                  reached, the f64 average of the per-frame survivor counts is >= min_average_number_of_states and either
 *                  increase_until_no_score_difference is 0 or t > min and Core::isAlmostEqual(score, previous score); factor <= 1: one pass.
 *                  A pass that pruned nothing gives what every later pass gives: those are counted, not run.
 *   result         the best final hypothesis by strict < over final weight + score in list order (the FIRST wins a tie, :408-419); per
 *                  frame the arc's label and score[hyp] - score[trace] (:438); no final state reached: score FLT_MAX, no alignment.
 * Limits of the search kernel (one workgroup per segment, the segment's states in LDS): at most AMX_ALIGN_MAX_STATES states and
 * AMX_ALIGN_MAX_EMISSIONS distinct emission indices per segment, at most AMX_ALIGN_MAX_OUT_ARCS arcs out of a state. */
#define AMX_ALIGN_MAX_STATES 2048
#define AMX_ALIGN_MAX_EMISSIONS 4096
#define AMX_ALIGN_MAX_OUT_ARCS 64
#define AMX_ALIGN_MAX_PASSES 4096
#define AMX_ALIGN_VITERBI 0
#define AMX_ALIGN_BAUM_WELCH 1
typedef struct {
    float  min_acoustic_pruning;                /* 50 */
    float  max_acoustic_pruning;                /* FLT_MAX */
    float  increment_factor;                    /* 2 */
    double min_average_number_of_states;        /* 0 */
    int    increase_until_no_score_difference;  /* 1 */
    int    n_best_pruning;                      /* INT_MAX; anything below is refused */
    int    mode;                                /* AMX_ALIGN_VITERBI; AMX_ALIGN_BAUM_WELCH is refused here: amx_bw_create has it */
    float  score_scale;                         /* 1: the scale of the acoustic model's scaled feature scorer */
} amx_align_cfg;
/* The graphs of a batch, on the host.  States of segment s are [state_offsets[s], state_offsets[s + 1]); arc_target and initial_state are
 * local to the segment.  Arcs of state i (global) are [arc_offsets[i], arc_offsets[i + 1]) in the reference's arc order. */
typedef struct {
    const int*           state_offsets;  /* [n_seg + 1] */
    const int*           initial_state;  /* [n_seg] */
    const unsigned char* is_final;       /* [states] */
    const float*         final_weight;   /* [states], read where is_final */
    const int*           arc_offsets;    /* [states + 1] */
    const int*           arc_target;     /* [arcs] */
    const int*           arc_emission;   /* [arcs] column of the score matrix */
    const int*           arc_label;      /* [arcs] what comes out: the allophone-state id */
    const float*         arc_weight;     /* [arcs] */
} amx_align_graphs;
typedef struct {
    float              score;           /* alignmentScore(); FLT_MAX when no final state was reached */
    int                reached_final;   /* 0 also for a segment that met a NaN */
    int                n_iterations;    /* passes as the reference counts them, the ones not run included */
    float              last_threshold;  /* the threshold of the last of them */
    double             average_states;  /* average number of state hypotheses after pruning, of the last pass (NaN for 0 frames) */
    unsigned long long state_sum;       /* its per-frame survivor counts added up */
} amx_align_result;
typedef struct amx_align amx_align;
void amx_align_default_cfg(amx_align_cfg* cfg); /* the reference's defaults (:473-528) */
/* Refused with AMX_ERR_UNSUPPORTED naming the parameter: mode = baum-welch (a handle of its own, amx_bw below); n_best_pruning < INT_MAX; an increment_factor that takes
 * more than AMX_ALIGN_MAX_PASSES steps from min to max.  With AMX_ERR_INVALID: min > max, or factor <= 1 with min != max (:543-550); a
 * threshold or scale that is NaN; min <= 0. */
int  amx_align_create(amx_ctx* ctx /* nullable: validation only */, const amx_align_cfg* cfg, amx_align** out);
void amx_align_destroy(amx_align* h);
/* Aligner::feed(vector) + getAlignmentFsa for n_seg segments in one launch sequence, one readback at the end.  Segment s = frames
 * [frame_offsets[s], frame_offsets[s + 1]) (host list, absolute rows) of scores_dev, label_dev, emission_dev and arc_score_dev.
 *   label_dev[t]      the label of the arc aligned to frame t; emission_dev[t] its emission index (what amx_gmm_accumulate_dev,
 *                     amx_scatter_accumulate_dev and margin_mixture_dev take); both -1 in a segment that reached no final state
 *   arc_score_dev[t]  nullable: score[hyp] - score[trace] of that arc, 0 in such a segment
 *   result[s]         host
 *   counters          nullable, host: [0] segments that met a NaN, [1] passes run on the device, [2] passes counted without running
 * Checked before anything is launched.  AMX_ERR_INVALID naming segment and index: an arc target, emission index or initial state out
 * of range, a NaN arc or final weight, offsets that decrease.  AMX_ERR_UNSUPPORTED: a segment with more states, distinct emissions or
 * arcs out of a state than the limits above.
 * Where the reference is undefined: a NaN candidate score met by the search (a NaN emission, or inf - inf) would make the outcome depend
 * on evaluation order; the segment is reported as not reached (n_iterations and last_threshold: the pass that met it) and counted. */
int  amx_align_viterbi_dev(amx_align* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const amx_align_graphs* graphs,
                           const float* scores_dev, int scores_ld, int n_columns, int32_t* label_dev, int32_t* emission_dev,
                           float* arc_score_dev, amx_align_result* result /*[n_seg]*/, unsigned long long counters[3]);

/* ------------------------------------------------------------------ Baum-Welch alignment on the score matrix: forward-backward, item lists */

/* amx_bw is one Search::Aligner in mode baum-welch (Search/Aligner.cc:169-196, 215-318, 385-405, 447-461, 594-630, 653-735, 766-781;
 * Fsa/Sssp.cc:67-202; Speech/Alignment.cc:426-578): the soft alignment of a batch of segments on the score matrix amx_align_viterbi_dev
 * reads.  Per frame it leaves a list of (allophone-state label, emission index, posterior weight), what Aligner::getAlignment returns.
 *   search         expansion, pruning rule and loop of thresholds are Viterbi's; a target's candidates score + (weight + emission) are
 *                  combined in the log semiring.  Here: the f64 log-sum min - log1p(sum exp(min - c)) over the state's incoming arcs in
 *                  the static by-target order, rounded to f32 once per state and frame (the reference collects in f32, pairwise, in list
 *                  order).  These f32 scores decide pruning, iterations and the reported score (finalStatePotential) only.
 *   posteriors     over the survivors of the last pass: forward and backward potentials in f64 (posterior64), arc weights
 *                  f32 (weight + emission); an arc's -log p = fw[source] + w + bw[target] - total
 *   items          exp(-.) summed per (frame, label) in a fixed order, divided by the frame's sum, rounded to f32; weights > 0 are kept.
 *                  Within a frame: decreasing weight, then increasing label.
 * A label must have one emission index within a segment (an acoustic model's emissionIndex() is a function of the label).
 * Not built: min-weight pruning, partial sums, extractAlignment's gamma, alignment files, word lattices, the statistics channel. */
#define AMX_BW_MAX_LABELS 4096 /* distinct labels per segment */
typedef struct {
    float  min_acoustic_pruning;                /* 50 */
    float  max_acoustic_pruning;                /* FLT_MAX */
    float  increment_factor;                    /* 2 */
    double min_average_number_of_states;        /* 0 */
    int    increase_until_no_score_difference;  /* 1 */
    int    n_best_pruning;                      /* INT_MAX; anything below is refused */
    float  score_scale;                         /* 1 */
    float  min_weight;                          /* 0; above FLT_MIN is refused (prunePosterior's second stage) */
    int    use_partial_sums;                    /* 0; 1 is refused */
} amx_bw_cfg;
typedef struct {
    float              score;           /* alignmentScore(): the f32 finalStatePotential of the last pass; FLT_MAX when no final state was reached */
    int                reached_final;   /* 0 also for a segment that met a NaN */
    int                n_iterations;
    float              last_threshold;
    double             average_states;
    unsigned long long state_sum;
    long long          n_items;         /* items of the segment */
    double             log_total;       /* bw[initial], -log of the trellis' total flow in f64; DBL_MAX where no final state was reached.  A reached
                                         * segment without frames reports its initial state's final weight and has no items */
} amx_bw_result;
typedef struct amx_bw amx_bw;
void amx_bw_default_cfg(amx_bw_cfg* cfg);
/* The search parameters are checked as amx_align_create checks them.  AMX_ERR_UNSUPPORTED naming the parameter: use_partial_sums = 1,
 * min_weight > FLT_MIN, n_best_pruning < INT_MAX, too many passes.  AMX_ERR_INVALID: a min_weight that is negative or not a number. */
int  amx_bw_create(amx_ctx* ctx /* nullable: validation only */, const amx_bw_cfg* cfg, amx_bw** out);
void amx_bw_destroy(amx_bw* h);
/* Search, posteriors and item combination for n_seg segments; one readback at the end (a second one only when the handle's item store
 * has to grow).  Segments, graphs, matrix and the checks before anything is launched are amx_align_viterbi_dev's; beyond them
 * AMX_ERR_UNSUPPORTED for a segment with more than AMX_BW_MAX_LABELS distinct labels and AMX_ERR_INVALID for a label with two emission
 * indices in one segment.
 *   item_offsets_dev  int64 [frame_offsets[n_seg] + 1], device: the items of matrix row t are [item_offsets_dev[t], item_offsets_dev[t + 1])
 *                     of the handle's item store (rows below frame_offsets[0] have none)
 *   result[s]         host
 *   counters          nullable, host: as amx_align_viterbi_dev
 * n_seg = 0: nothing is launched and nothing is written, item_offsets_dev included; amx_bw_n_items is 0.
 * Added rules: a NaN candidate, or inf - inf in a log-sum, ends the segment, which is reported as not reached and counted; a segment that
 * reaches no final state has no items and score FLT_MAX; so has one without frames. */
int  amx_bw_align_dev(amx_bw* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const amx_align_graphs* graphs, const float* scores_dev,
                      int scores_ld, int n_columns, int64_t* item_offsets_dev, amx_bw_result* result /*[n_seg]*/, unsigned long long counters[3]);
/* The items of the last amx_bw_align_dev call, copied out of the handle's store (device to device, on the context's stream): frame
 * (the matrix row), label, emission index, weight; weight_f64_dev (nullable): the same values widened, what
 * amx_gmm_accumulate_weighted_dev takes as weight_dev.  Ordered by frame, then decreasing weight, then label.  A capacity below the
 * number of items is AMX_ERR_INVALID naming the needed count. */
long long amx_bw_n_items(const amx_bw* h);
int  amx_bw_items_dev(amx_bw* h, long long capacity, int32_t* frame_dev, int32_t* label_dev, int32_t* emission_dev, float* weight_dev,
                      double* weight_f64_dev);
/* dst[i * dst_ld + d] = src[row_dev[i] * src_ld + d], d < dim, i < n: the feature rows of the items, so that
 * amx_gmm_accumulate_weighted_dev(..., T = n_items, mixture_dev = emission, weight_dev = weight_f64) takes them unchanged.  The row
 * numbers are on the device and are not checked. */
int  amx_gather_rows_dev(amx_ctx* ctx, const float* src_dev, int src_ld, int dim, long long n, const int32_t* row_dev, float* dst_dev, int dst_ld);

/* ------------------------------------------------------------------ Linear-segmentation alignment: delimiter search, flat start */

/* amx_linseg is one Speech::LinearSegmenter (Speech/AlignmentWithLinearSegmentation.cc:30-350; the node speech-linear-segmentation, what
 * AlignmentWithLinearSegmentationNode::work runs per segment): the first alignment of a training, made without a model.  A two-Gaussian
 * silence / speech / silence delimiter (Bridle, Sedgwick, ICASSP'77) runs over ONE f32 value per frame, the energy stream, and the
 * segment's flat allophone-state sequence is spread linearly over the speech part with the silence state on both sides.  Per segment of
 * N frames with n_states states:
 *   checks       no states or N = 0: NO_STATES (isAlignmentValid, :311-313, :413-417); N < minimum_segment_length: TOO_SHORT (:316-317);
 *                N > maximum_segment_length: TOO_LONG (:318-319); then delimitation and spread; index - previousIndex > 2: JUMP
 *                (:333-336); a last index that is not n_states - 1: MISMATCH (:340-344)
 *   feed         (:61-71) x widened to f64; M_[i] = M_[i-1] + x, Q_[i] = Q_[i-1] + (x * x + f / 2) / f (penalty f = 0: + x * x): two
 *                sequential f64 chains in frame order, M_[0] = Q_[0] = 0
 *   likelihood   (:103-120) logLikelihood(ib, ie) as written: s1 = (f64)(u32)(ib - 1 + N - ie), the variances floored at 0.5, the double
 *                logarithm, and DBL_MAX unless (m1 / s1) < (m2 / s2) and (f32)(ie - ib) >= minimum_speech_proportion * (f32)N (an f32 product)
 *   delimiter    (:145-182) proportion == 1: (0, N - 1); N == 1: (0, 0); else number_of_iterations times ib over [2, iEnd - 1) against iEnd,
 *                then ie over [iBeg + 1, N - 1) against iBeg, in u32 arithmetic, x_min carried across the iterations, a candidate wins
 *                by strict <: of equal candidates the first.  Starts: iBeg = 1, iEnd = N - 1, x_min = DBL_MAX.
 *   sietill      should_use_sietill (:200-245): iBeg = 1, iEnd = N; per iteration x_min = DBL_MAX, ib over [2, N) except iEnd with
 *                logLikelihood(min(iEnd, ib), max(ib, iEnd)), then ie over [2, N) except iBeg likewise, then the pair is put in order.  No
 *                N == 1 shortcut, and iEnd may stay N: the speech part then ends with the segment's last frame.
 *   spread       (:325-347) begin = iBeg - 1, end = iEnd - 1; slope = (f32)(n_states - 1) / (f32)max(end - begin, 1);
 *                index = (u32)round(slope * (f32)(t - begin)) for t in [begin, end]; the silence label on [0, begin) and (end, N)
 * Added rule (the reference raises an error when Q_ overflows, :69-70, and is undefined on NaN): an energy that is not finite, or an M_ or
 * Q_ that leaves the finite range, gives NONFINITE.  Any reason but OK writes -1 to every label_dev / emission_dev row of the segment, which
 * amx_gmm_accumulate_dev and amx_scatter_accumulate_dev skip.
 * amx_set_contract selects which build of the reference is followed: its -march=native build contracts logLikelihood's `xsil + xspe`
 * (xspe's product s2 * log(.) goes into the sum as one fused multiply-add); tests/golden/ref_linseg.npz records which arrays the two
 * builds compute differently.  It contracts feed's `xx * xx + f_ / 2.0` as well, which changes no bit: xx is a widened f32, its square is
 * exact in f64.
 * The logarithm is the device library's double log (at most 1 ulp from the exact value), glibc's is the reference's: a delimitation whose
 * winning candidate is closer than 2^-48 of the larger |s * log(.)| term to another one may differ.
 * Not built: the flat model itself (the adapter walks the allophone-state graph builder's automaton, setModel :293-305), the silence
 * index, model and alignment caches, timestamps, the statistics channel. */
enum { AMX_LINSEG_OK = 0, AMX_LINSEG_TOO_SHORT, AMX_LINSEG_TOO_LONG, AMX_LINSEG_NO_STATES, AMX_LINSEG_JUMP,
       AMX_LINSEG_MISMATCH, AMX_LINSEG_NONFINITE, AMX_LINSEG_N_REASONS };
typedef struct {
    int    number_of_iterations;        /* 3    delimiter.number-of-iterations (:81-84) */
    double penalty;                     /* 100  delimiter.penalty, 0 = none (:86-89) */
    float  minimum_speech_proportion;   /* 0.7  delimiter.minimum-speech-proportion, within [0, 1] (:91-94) */
    int    should_use_sietill;          /* 0    (:259-262) */
    int    minimum_segment_length;      /* 1    (:254-257) */
    int    maximum_segment_length;      /* INT_MAX (:249-252) */
} amx_linseg_cfg;
typedef struct {
    int    reason;                      /* AMX_LINSEG_* */
    int    speech_begin, speech_end;    /* 0-based, inclusive; -1 when not computed */
    double score;                       /* the final x_min; DBL_MAX if no candidate ever won, a shortcut was taken or nothing was computed */
} amx_linseg_result;
typedef struct { /* host: the flat model of every segment, LinearSegmenter::setModel's states_ */
    const int* state_offsets;  /* [n_seg + 1] */
    const int* state_label;    /* [states] allophone-state ids in path order */
    const int* state_emission; /* [states] emission index of each */
    int        silence_label, silence_emission;
} amx_linseg_models;
typedef struct amx_linseg amx_linseg;
void amx_linseg_default_cfg(amx_linseg_cfg* cfg);
/* AMX_ERR_INVALID naming the field: a penalty or proportion that is not a number, a negative penalty, a proportion outside [0, 1],
 * negative iterations or lengths.  AMX_ERR_UNSUPPORTED: more than 4096 iterations (the kernel stops at the first iteration that changes
 * nothing, which every later one would repeat; the limit bounds a search that never settles). */
int  amx_linseg_create(amx_ctx* ctx /* nullable: validation only */, const amx_linseg_cfg* cfg, amx_linseg** out);
void amx_linseg_destroy(amx_linseg* h);
/* The whole node for n_seg segments in one launch, one readback at the end.  Segment s = frames [frame_offsets[s], frame_offsets[s + 1])
 * (host list, absolute rows): its energies are energy_dev[t * energy_ld], its labels label_dev[t] and emission_dev[t] (int32).
 *   result[s]   host
 *   counters    nullable, host: counters[r] = segments of this call with reason r
 * Checked before anything is launched, AMX_ERR_INVALID naming the field: offsets that are negative or decrease, state offsets that do not
 * start at 0 or decrease, a negative label or emission index, energy_ld < 1, NULL buffers where there are frames; frame_offsets[n_seg]
 * must stay below 2^31.  A handle without a context returns AMX_ERR_STATE after these checks. */
int  amx_linseg_align_dev(amx_linseg* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const amx_linseg_models* models,
                          const float* energy_dev, int energy_ld /* floats between two frames' values */,
                          int32_t* label_dev, int32_t* emission_dev, amx_linseg_result* result /*[n_seg]*/,
                          unsigned long long counters[AMX_LINSEG_N_REASONS] /* nullable */);
/* Debug read of the handle's workspace after a call: M_ and Q_ of segment s of that call, N + 1 doubles each (host buffers, nullable). */
int  amx_linseg_chains(amx_linseg* h, int segment, double* m, double* q);

/* ------------------------------------------------------------------ Decision-tree state tying: device example sums and split search */

/* The step between a monophone and a triphone system: Speech::FeatureAccumulator builds one Cart::Example per allophone state from the
 * aligned corpus (Speech/DecisionTreeTrainer.cc:54-90), Cart::DecisionTreeTrainer grows the tree (Cart/DecisionTreeTrainer.cc:353-801)
 * with StateTyingDecisionTreeTrainer::LogLikelihoodGain as its scorer (Speech/DecisionTreeTrainer.cc:134-250).
 *
 * ACCUMULATION.  The accumulator is ONE caller-owned flat f64 device buffer [n_labels x (1 + 2 dim)], zeroed by the caller before the
 * first call; row id = [nObs, sum[dim], sumSq[dim]] is the Example of allophone state id (Cart/Example.hh: FloatBox(2, nCols)).  Ranks
 * combine it with amx_comm_all_reduce_f64_dev.  Per frame t with id = label_dev[t] (what amx_align_*, amx_bw_* and amx_linseg_align_dev
 * leave there) and weight w (weight_dev NULL: 1), processAlignedFeature (:58-90):
 *     id == -1 or w == 0: nothing;  nObs[id] += w;  sum[id][c] += (f64)x * w;  sumSq[id][c] += (f64)(x * x) * w   (x * x an f32 product;
 *     Mm::Weight is f64, Mm/Types.hh:30)
 * Per (id, c) this is one chain over the frames in ascending order that CONTINUES from the value in the buffer: a corpus fed in order,
 * cut into calls anywhere, gives the reference's bits.  No floating-point atomics; nothing depends on the launch.  The two `+= . * w`
 * are contraction sites of the reference's default build: amx_set_contract(AMX_CONTRACT_FMA) makes them fused multiply-adds.  With
 * w = 1 both settings give the same bits (the product is exact).
 * Labels are checked on the device before anything is written: an id outside [0, n_labels) other than -1 returns AMX_ERR_INVALID naming
 * the first such frame, acc_dev untouched (amx_nntrain_accumulate_dev's convention).  The call synchronises the context's stream.
 * Expected cost (not a measurement): the longest label's chain, silence, at one dependent f64 operation per frame. */
size_t amx_cart_accumulator_size(int n_labels, int dim);   /* doubles */
int    amx_cart_accumulate_dev(amx_ctx* ctx, const float* feats_dev, int feats_stride /* floats between two frames */, int dim, int T,
                               const int32_t* label_dev, const double* weight_dev /* nullable, [T] */, int n_labels, double* acc_dev);

/* TRAINING.  Questions, property maps and the XML files of examples and trees stay with the adapter (Cart::Question and its kin are
 * RASR objects): it evaluates every question once on every example and hands over bits.
 *   problem   n_examples rows of the accumulator (the caller drops labels it has not seen): n_obs[E], values[E x 2 dim] (sum, then sumSq),
 *             and answers[n_questions x ceil(E / 32)], bit (e & 31) of word e / 32 of row q = (question q (properties of e) == TRUE).
 *             Host arrays; the library uploads them once per training.
 *   plan      TrainingPlan (Cart/DecisionTreeTrainer.hh:130-170): max_leaves and steps, each with an action, min_obs, min_gain and a
 *             list of rows of `answers` (its questions, in the order of its question list); variance_clipping is the scorer's.
 *             randomize is nRandomQuestion: above 1 it is AMX_ERR_UNSUPPORTED (the reference seeds the choice with time(0), :219).
 * What is followed operation by operation:
 *   lists     a node's example list is ordered; a split is a stable partition (:498-504); rollbackSplit leaves left + right concatenated
 *             for the next step (:599-611); a node's question-id list loses the used entry by swap with the back (:575-576), so ties in
 *             the gain depend on that order
 *   counts    nLeftObs / nRightObs and the root's nObs are u32 that take f64 additions: every addition truncates (:360, :458, :462)
 *   skips     node.nObs < 2 * minObs (u32 product): no split (:398); a side below minObs (:471); strict: a side of 0 observations or a
 *             gain of 0 (:473, :486); gain < minGain (:484); a negative gain is skipped, and counted as an error unless f32(gain) is
 *             within 20 ulps of 0 (:479-483; the reference's error() goes on as well)
 *   winner    SplitHypothesesManager::push with one slot (:249-258): the first question with the strictly largest gain
 *   queue     Core::PriorityQueue's own heap moves (Core/PriorityQueue.hh:55-108), equal gains included; the leaf limit
 *             nLeaf + nodes + splits < maxLeaves before each commit (:635, :662, :670); split, partition and cluster (:622-676)
 *   numbers   order numbers in insertSplit (:534-535); class ids in commitNode's pre-order (:706-726) with the RIGHT child first: the two
 *             recursive calls are arguments of one call (:712-714), their order is the compiler's, and the reference's GCC build
 *             evaluates them from the right (found by tests/golden/make_cart_golden.py, held by tests/golden/ref_cart.npz)
 *   score     logLikelihood (Speech/DecisionTreeTrainer.cc:205-232): plain f64 chains in list order from +0.0, mu = s / n,
 *             var = q / n - mu * mu, clipped, ll an ascending chain of ::log, (0.5 n)(d + d log(pi + pi) + ll); gain = father - (left + right).
 *             amx_set_contract(AMX_CONTRACT_FMA): var = fma(-mu, mu, q / n) and d + d * log(.) = fma(d, log(.), d), the sites a
 *             contracting build fuses.
 * The sums and counts of every (node, question) come from the device (cart.hip), in the reference's order.  The device's log is not
 * glibc's, so its gain is a SCREEN: a question goes through the host's ::log -- on the device's sums -- unless the screen decides it by
 * more than a margin derived from the log's error bound.  exact_all = 1 sends every question through the host
 * (the slow reference mode, and the check on the margin).  splitNode depends on the node's list, its question list and the step alone,
 * so the children of queued splits are evaluated ahead of the queue in wide launches; this changes no result.
 * Refused: AMX_ERR_INVALID naming the field for NULL arrays, sizes below their minimum, a negative or non-finite n_obs, an unknown action,
 * a question row outside the matrix; AMX_ERR_UNSUPPORTED for randomize > 1, dim > 1024 and a total n_obs of 2^32 or more (the reference
 * counts in 32 bits).  ctx == NULL: AMX_ERR_STATE after these checks. */
enum { AMX_CART_SPLIT = 0, AMX_CART_PARTITION = 1, AMX_CART_CLUSTER = 2 };
typedef struct {
    int             n_examples, dim, n_questions;
    const double*   n_obs;    /* [E] */
    const double*   values;   /* [E x 2 dim] */
    const uint32_t* answers;  /* [Q x ceil(E / 32)] */
} amx_cart_problem;
typedef struct {
    int        action;        /* AMX_CART_* */
    unsigned   min_obs;       /* 0 */
    double     min_gain;      /* 0 */
    int        randomize;     /* 1 */
    int        n_questions;
    const int* questions;     /* rows of answers */
} amx_cart_step;
typedef struct {
    unsigned             max_leaves;          /* UINT_MAX */
    int                  n_steps;
    const amx_cart_step* steps;
    double               variance_clipping;   /* 0 */
    int                  exact_all;           /* 0 */
} amx_cart_plan;
typedef struct { /* in `order` */
    int      step, row;       /* the question: the step and its row of answers; -1, -1 for a leaf */
    int      left, right;     /* orders of the children; -1 for a leaf */
    unsigned depth, n_obs;
    double   score;
    int      class_id;        /* -1 for an inner node */
} amx_cart_node;
typedef struct { /* one committed split (insertSplit's log message) */
    int      node, step, row;
    unsigned depth;
    double   gain, total_gain;
} amx_cart_commit;
typedef struct { /* QuestionStatistic (Cart/DecisionTreeTrainer.cc:140-156) of every question of every step that ran */
    int      step, row;
    unsigned count;
    double   min_gain, sum_gain, max_gain;
    unsigned min_depth, sum_depth, max_depth;
} amx_cart_qstat;
typedef struct {
    int      n_nodes, n_leaves, n_commits, n_question_stats, n_examples;
    unsigned n_obs;
    double   initial_score, total_gain;
    unsigned long long negative_gain_errors, items_screened, items_reevaluated, launches;
} amx_cart_info;
typedef struct amx_cart_tree amx_cart_tree;
int  amx_cart_train(amx_ctx* ctx, const amx_cart_problem* problem, const amx_cart_plan* plan, amx_cart_tree** out);
void amx_cart_tree_destroy(amx_cart_tree* tree);
int  amx_cart_tree_info(const amx_cart_tree* tree, amx_cart_info* info);
/* host buffers, each nullable: nodes[n_nodes], classes[n_examples] (example -> class id), log[n_commits], question_stats[n_question_stats] */
int  amx_cart_tree_get(const amx_cart_tree* tree, amx_cart_node* nodes, int32_t* classes, amx_cart_commit* log, amx_cart_qstat* question_stats);
/* the split search's launch shape for a dimension: examples per LDS stage, questions per workgroup (tests pick their sizes around them) */
void amx_cart_kernel_shape(int dim, int* stage_examples, int* tile_questions);

/* ------------------------------------------------------------------ Quantile equalisation: device grid search, quantile files, apply */

/* amx_quanteq is one Signal::QuantileEqualization (Signal/QuantileEqualization.{hh,cc}) in SEGMENT MODE (length = right = INT_MAX): the
 * arithmetic of the node `signal-quantile-equalization` (Signal/Module.cc:145) for a batch of segments whose [frames x dim] f32 feature
 * matrix is on the device.  Per segment of T frames, once, over all T frames (QuantileEqualization.cc:149-307):
 *   quantiles   per channel d the column is sorted; currentQuantile[i * dim + d] = sorted[(u32)(i * (T - 1) / nq)], i = 0 .. nq.
 *   alpha/gamma maximalQuantile = max(of * tq[nq], of * cq[nq]) (f32); scaled_i = max(tq[i], cq[i]) / maximalQuantile (f32);
 *               transformed_i = (f32)((f64)maximalQuantile * ((f64)a * pow((f64)scaled_i, (f64)g) + (1. - (f64)a) * (f64)scaled_i)), pow the
 *               double function; distance = sum over i = 1 .. nq - 1 of (transformed_i - tq[i])^2 in f32.  The grid is what the
 *               reference's loop `for (f32 a = lo; a <= hi; a += (f64)step)` visits ([0, 1] for alpha, [1, 3] for gamma; 201 x 201 with
 *               the default steps, which are (f64)(f32)0.005 and (f64)(f32)0.01); the winner is the first point, alpha outer, whose
 *               distance is < the best so far, starting from FLT_MAX: NaN and infinite distances never win, and where none wins
 *               alpha = 0, gamma = 1.  The interior quantiles are then replaced by their transformed values.
 *   lambda/rho  (combination) over [0, 0.5]^2, step delta_lambda_and_rho: (1. - l - r) * cq[i][d] + l * cq[i][max(d - 1, 0)] +
 *               r * cq[i][min(d + 1, dim - 1)] on the TRANSFORMED quantiles (the first product f64, the other two f32, summed in f64), narrowed, distance as above plus (l * l + r * r) * beta.
 *   apply       x -> the power function of x / maximalQuantile under the winning (alpha, gamma); then the neighbour combination, all
 *               channels read from the frame before the combination; then - mean and, with variance, / deviation, where
 *               mean = (f32)(sum / T), deviation = (f32)sqrt((sumSquare - sum * sum / T) / T) are f64 sums over the transformed frames from
 *               the oldest to the newest.  variance without mean does nothing (:330-335), and its reported deviation is 0.
 * Division by a zero maximalQuantile or deviation gives inf / NaN where the reference gives them.
 * amx_set_contract selects which build of the reference is followed: its -march=native build contracts `distance += tmp * tmp`,
 * `a * pow + (1. - a) * scaled` (the first product), the f64 product of the combination, `l * l + r * r`, the penalty's
 * `distance += ... * beta` and `sumSquare += x * x`.
 * Not copied from the reference: only the first object of a process reads its training file there (`firstcall` is a function-local
 * static, :29); here every handle gets its training quantiles.
 * Bounds: dim <= AMX_QUANTEQ_MAX_DIM; number_of_quantiles 1 .. AMX_QUANTEQ_MAX_QUANTILES; a grid side of at most AMX_QUANTEQ_MAX_GRID_SIDE
 * points; a segment of at most AMX_QUANTEQ_MAX_SEGMENT_FRAMES frames (the column is sorted in LDS). */
#define AMX_QUANTEQ_MAX_DIM 4096
#define AMX_QUANTEQ_MAX_QUANTILES 16
#define AMX_QUANTEQ_MAX_GRID_SIDE 4096
#define AMX_QUANTEQ_MAX_SEGMENT_FRAMES 16384
typedef struct {
    int   quantiles;             /* `quantiles`, 1 */
    int   combination;           /* `combination`, 0 */
    int   estimate;              /* `estimate`, 0: 1 gives a handle for amx_quanteq_estimate_dev only */
    int   mean;                  /* `mean`, 1 */
    int   variance;              /* `variance`, 0 */
    int   number_of_quantiles;   /* `numberOfQuantiles`, 4 */
    float overestimation_factor; /* `overestimationFactor`, 1 */
    float delta_alpha;           /* `deltaAlpha`, .005: f32 as the reference's setter takes it */
    float delta_gamma;           /* `deltaGamma`, .01 */
    float delta_lambda_and_rho;  /* `deltaLambdaAndRho`, .005 */
    float beta;                  /* `beta`, .05 */
    int   pool_quantiles;        /* `poolQuantiles`, 1: acts in amx_quanteq_quantiles_read, whose result create takes */
    int   piecewise_linear;      /* `piecewiseLinear`, 0; 1 is refused */
    long  length;                /* `length`: anything below INT_MAX is the sliding-window mode, refused */
    long  right;                 /* `right`: likewise */
} amx_quanteq_cfg;
typedef struct amx_quanteq amx_quanteq;
void amx_quanteq_default_cfg(amx_quanteq_cfg* cfg);
/* training_quantiles: [(nq + 1) x dim], element [i * dim + d], as amx_quanteq_quantiles_read returns them; NULL with quantiles = 0 or
 * estimate = 1.  AMX_ERR_UNSUPPORTED, naming the parameter: length / right below INT_MAX, piecewise_linear, a step <= 0 (the reference
 * loops forever) or a grid of more than AMX_QUANTEQ_MAX_GRID_SIDE points a side, number_of_quantiles outside its bounds. */
int  amx_quanteq_create(amx_ctx* ctx /* nullable: configuration and grids only */, int dim, const amx_quanteq_cfg* cfg, const float* training_quantiles,
                        amx_quanteq** out);
void amx_quanteq_destroy(amx_quanteq* h);
/* the grid tables as the reference's loops visit them: which = 0 alpha, 1 gamma, 2 lambda and rho; values nullable */
int  amx_quanteq_grid(const amx_quanteq* h, int which, int* n, float* values);
/* The training quantile file (text): per channel one line `"%i " d`, then `"%f "` for i = 0 .. nq, then "\n"
 * (writeEstimatedQuantilesToFile, :103-119: value = sums[i * dim + d] / (u32)count).  read (:70-101) fills out[(nq + 1) x dim]; with pool
 * each quantile is replaced by its f32 average over the channels (f32 sum in channel order, divided by dim).  A file that cannot be
 * opened or holds fewer numbers is AMX_ERR_INVALID. */
int  amx_quanteq_quantiles_read(const char* path, int dim, int nq, int pool, float* out);
int  amx_quanteq_quantiles_write(const char* path, int dim, int nq, const double* sums, unsigned long long count);
/* The whole node for segments s = frames [frame_offsets[s], frame_offsets[s + 1]) (host list, absolute rows) of in_dev[t * in_ld + d] into
 * out_dev[t * out_ld + d]; columns >= dim are neither read nor written; out_dev may be in_dev with out_ld == in_ld.  An empty segment does
 * nothing.  params_host (nullable): [n_seg x dim * (6 + nq + 1)] floats, per segment alpha[dim], gamma[dim], lambda[dim], rho[dim],
 * mean[dim], deviation[dim], then the (nq + 1) x dim current quantiles AS FIRST TAKEN (before the interior ones are replaced); all zero for
 * an empty segment.  With quantiles = 1 the call synchronises the stream once after the quantile kernel, and again when params_host is asked
 * for.  A value of columns < dim that is not finite fails the call with AMX_ERR_INVALID naming the first (segment, channel), and nothing
 * is written (std::sort is undefined on NaN).  -0 sorts before +0 (the reference leaves their order to the sort).  A segment of more than
 * AMX_QUANTEQ_MAX_SEGMENT_FRAMES frames is AMX_ERR_UNSUPPORTED, naming it. */
int  amx_quanteq_apply_dev(amx_quanteq* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const float* in_dev, int in_ld, float* out_dev,
                           int out_ld, float* params_host);
/* estimate = 1 (:171-172, :314-317): the quantiles of every non-empty segment, taken on the device, are added to the handle's f64 sums on the
 * host in segment order, one count per segment; any split of the segments over calls gives the same sums.  The node's output stream in
 * this mode is not built.  amx_quanteq_estimate_result copies the sums [(nq + 1) x dim] and the count for amx_quanteq_quantiles_write. */
int  amx_quanteq_estimate_dev(amx_quanteq* h, int n_seg, const long* frame_offsets /*[n_seg+1]*/, const float* in_dev, int in_ld);
int  amx_quanteq_estimate_result(const amx_quanteq* h, double* sums, unsigned long long* count);

/* ------------------------------------------------------------------ mixture-set text files (.pms) */

/* Reader / writer of RASR's text mixture-set format, "#Version: 2.0" (Mm/MixtureSet.cc:141-216,
 * Mm/Mixture.cc:80-105, Mm/MixtureSetTopology.cc:19-30, Mm/GaussDensity.cc:25-70).  Version < 2.0
 * files carry linear weights (converted with log), covariances are stored as (variance, weight)
 * pairs whose product is the diagonal.  The returned object owns its arrays; amx_mixture_set_view
 * fills an amx_gmm_model with pointers into it (scales set to 1). */
int  amx_pms_read(const char* path, amx_mixture_set** out);
int  amx_pms_write(const amx_gmm_model* model, const char* path);
int  amx_mixture_set_view(const amx_mixture_set* ms, amx_gmm_model* view);
void amx_mixture_set_destroy(amx_mixture_set* ms);

/* ------------------------------------------------------------------ feed-forward NN scorer */

/* AMX_ACT_ELU: RASR's `elu` layer with its alpha fixed at 1 (Nn/ActivationLayer.cc:331-396, Math::FastMatrix<f32>::elu,
 * Math/FastMatrix.hh:1658-1667): x < 0 ? exp(x) - 1 : x, the exponential is std::exp on a float (expf); a NaN stays NaN. */
enum { AMX_ACT_NONE = 0, AMX_ACT_RELU = 1, AMX_ACT_SIGMOID = 2, AMX_ACT_TANH = 3, AMX_ACT_ELU = 4 };
/* MFMA input type; accumulation is always f32.  AMX_PREC_BF16X3 = split bf16: every operand is hi + lo (two bf16 values) and a
 * product is taken as hi hi + lo hi + hi lo -- three bf16 MFMA products, ~2^-16 relative error per product: the mode that meets
 * the 1e-4 bar of the f32 reference (Math::gemm<f32>, Math/Blas.hh:402-420) at a third of the bf16 rate */
enum { AMX_PREC_FP32 = 0, AMX_PREC_BF16 = 1, AMX_PREC_BF16X3 = 2, AMX_PREC_F16MX = 3 };
/* AMX_PREC_F16MX (round 4): every operand v is h = f16(v) plus an MX-fp6 image of the residual v - h (OCP e2m3, one e8m0 scale per
 * 32 k); a product is h h + fp6(h) fp6(w - h_w) + fp6(v - h_v) fp6(h_w) -- one f16 MFMA product and ONE block-scaled fp6 x fp6 MFMA
 * product for both cross terms (the fp6 image of h is converted from the f16 fragments in registers): 1.5 units of matrix time
 * per product instead of split bf16's 3, worst error 0.03 of the 1e-4 bar on BASELINE config 4 (profiles/r04/emulation_f16_f8.json,
 * tests/test_ffnn_f16mx_gpu.py).
 * Limits: weights and activations must stay inside the f16 range (|v| < 65520, and finite): amx_ffnn_create refuses such weights; a
 * pass that meets such a feature or hidden activation (inf and NaN included) FAILS, its scores are not valid:
 *   amx_ffnn_score (host buffers; it waits for its results) returns AMX_ERR_STATE for that very pass;
 *   the *_dev entry points only enqueue work: call amx_ffnn_wait_dev(h) behind a pass and before its scores are used -- it waits for
 *     the handle's stream and returns AMX_ERR_STATE if the pass (or an earlier one) left the range.  rasr_amd/host/
 *     BatchFeatureScorer.hh does so before a row of the block reaches the decoder (Nn/BatchFeatureScorer.cc:148-171 hands out scores
 *     of a batch it has computed synchronously);
 *   the flag is sticky: every later call on the handle returns AMX_ERR_STATE too (create the scorer with AMX_PREC_BF16X3, which
 *     has no such limit). */

typedef struct {
    int                 n_layers;
    const int*          in_dim;     /* [n_layers] */
    const int*          out_dim;    /* [n_layers] */
    const float* const* W;          /* [n_layers] each [out x in] row-major (== RASR weights_[0], [in x out] col-major) */
    const float* const* bias;       /* [n_layers] each [out] */
    const int*          activation; /* [n_layers] AMX_ACT_*; last layer must be AMX_ACT_NONE */
    const float*        log_prior;  /* nullable [out_last]  (Nn::Prior) */
    float               prior_scale;/* priori-scale alpha */
    int                 precision;  /* AMX_PREC_* */
    /* Nn::ClassLabelWrapper (Nn/ClassLabelWrapper.cc:21-70, used by Nn/BatchFeatureScorer.cc:148-171 and Nn/FeatureScorer.cc):
     * emission (class) e reads network output class_to_output[e]; -1 = disregarded class (`disregard-classes`), which scores
     * Core::Type<f32>::max.  NULL = identity (n_classes is then ignored).  The mapping must be one-to-one and cover every
     * output ("no one-to-one correspondence between network outputs and classes!"); scores are [T x n_classes]. */
    int                 n_classes;
    const int*          class_to_output;
    /* "key=value,key=value" (NULL: defaults); keys and values are checked by amx_ffnn_create like amx_gmm_model.tuning's.
     * Two keys change RESULTS (within the 1e-4 bar of the f32 reference either way):
     *   ksplit=4 (AMX_PREC_F16MX; default 1)  passes of at most 256 frames -- a decoder's ring-buffer fill -- split the K of every
     *        2048-wide layer over four workgroups per tile (two launches: partial sums, then ((P0 + P1) + P2) + P3 and the epilogue):
     *        four times as many CUs pull operands, a 256-frame fill of BASELINE config 4's network takes 0.146 instead of 0.170 ms.
     *        Another association of the sum over k than the default (one accumulator, ascending k): scores differ from the default's
     *        by f32 rounding and are bit-identical among all passes that are split; larger passes of the same handle run the default
     *        order.  Without it, scoring a segment in pieces gives the bits of scoring it whole.
     *   mx_fallback=auto|off (AMX_PREC_F16MX; default auto)  auto: heavy-tailed weights compute in split bf16 (amx_ffnn_precision).
     * Kernel selection for A/B runs and tests -- every tile configuration of a precision gives bit-identical scores: tile=N (GEMM tile
     * configuration: 0 128x128, 2 256x256 with all waves in phase, 8 256x256 with the ping-pong K loop (f16mx; the default for large
     * batches since round 5), 9 256x256 with ONE self-pipelined wave per SIMD (f16mx; measured 6 % behind 8, opt-in), 3 128x64 one tile per
     * CU, 6 128x64 two per CU, 4 / 5 / 7 K-loop variants of 2, 11 / 12 K-loop variants of 3, 14 (f16mx) hidden layers on 64x64 tiles with four
     * K-tiles per barrier -- the default for fills that leave half the CUs without a 128x64 tile; default by layer shape),
     * graph=1 (HIP-graph replay of repeated small passes; off by default since round 6, see amx_gmm_model.tuning), persistent=0, group=TxN (tiles per XCD-aware super-tile), chunk=N (frames per
     * internal pass, >= 256), stagger=N (f16mx output layer of a large batch: XCD x starts x * N * 10 ns late; default 0). */
    const char*         tuning;
} amx_ffnn_model;

int  amx_ffnn_create(amx_ctx* ctx, const amx_ffnn_model* model, amx_ffnn** out);

/* Layer types of Nn::NeuralNetwork (Nn/NeuralNetworkLayer.cc:34-56) beyond the linear + activation chain of amx_ffnn_model; an
 * optional descriptor next to the model, which stays as it is.
 * Preprocessing layers in front of layer 0, applied in pre_type order to the f32 features while they are packed for the first GEMM
 * (no extra pass over the frames); they stack (e.g. log, then mean and variance):
 *   AMX_NN_PRE_LOGARITHM          `logarithm` (Nn/PreprocessingLayer.cc:40-74): FastMatrix::log -> Math::vr_log
 *                                 (Math/FastVectorOperations.hh:86-90), the unqualified `log` on a float, which resolves to ::log(double)
 *                                 there (the same header and overload set as mt_vr_exp): (float)log((double)x).
 *   AMX_NN_PRE_MEAN_AND_VARIANCE  `mean-and-variance-normalization` (Nn/PreprocessingLayer.cc:86-177, `mean-file` and
 *                                 `standard-deviation-file`, f32 vectors: amx_nn_vector_read_f32): addToAllColumns(mean, -1) then
 *                                 divideRowsByScalars(stddev) = scal((f32)1 / s) (Math/FastMatrix.hh:1356-1361,1439-1444):
 *                                 x' = (x - m) * r with r = 1.0f / s.  A zero or negative s is accepted, as the reference does.
 * `maxoutvar` (Nn/ActivationLayer.cc:404-520, Math::FastMatrix::maxoutvar, Math/FastMatrix.hh:840-860): maxout_groups[l] = G > 0
 * puts a maxout behind layer l, which then computes maxout(act_l(W_l x + b_l)) with G outputs (in_dim[l + 1] == G).  Output g is
 * the maximum of its group of consecutive units: the first element is the start value and a later one replaces it only if it is
 * strictly greater (a NaN in first position stays, a later NaN never wins).  Group sizes: maxout_sizes[l] (`maxout-sizes`, a
 * Math::Vector<u32> file: amx_nn_vector_read_u32), each >= 1 and adding up to out_dim[l]; NULL = `maxout-size`, out_dim[l] / G each
 * (it must divide).  No maxout after the output layer.
 * ext == NULL is amx_ffnn_create.  Invalid descriptors return AMX_ERR_INVALID with a message naming the layer.  The network's hidden
 * dimension (amx_ffnn_hidden_dim) is the width after the last hidden layer's maxout; a network without hidden layers exports its
 * preprocessed input from amx_ffnn_forward_hidden_dev. */
enum { AMX_NN_PRE_LOGARITHM = 1, AMX_NN_PRE_MEAN_AND_VARIANCE = 2 };
#define AMX_NN_MAX_PRE 4
typedef struct {
    int                 n_pre;          /* preprocessing layers in front of layer 0, applied in this order (0..AMX_NN_MAX_PRE) */
    const int*          pre_type;       /* [n_pre] AMX_NN_PRE_* */
    const float* const* pre_mean;       /* [n_pre] each [in_dim[0]] for AMX_NN_PRE_MEAN_AND_VARIANCE, else NULL */
    const float* const* pre_stddev;     /* [n_pre] each [in_dim[0]] for AMX_NN_PRE_MEAN_AND_VARIANCE, else NULL */
    const int*          maxout_groups;  /* nullable [n_layers]: 0 = none, G > 0 = maxoutvar with G outputs behind layer l */
    const int* const*   maxout_sizes;   /* nullable [n_layers]: [G] group sizes, NULL = out_dim[l] / G each */
} amx_ffnn_layers;
int amx_ffnn_create_ex(amx_ctx* ctx, const amx_ffnn_model* model, const amx_ffnn_layers* ext, amx_ffnn** out);
void amx_ffnn_destroy(amx_ffnn* h);
int  amx_ffnn_input_dim(const amx_ffnn* h);
int  amx_ffnn_output_dim(const amx_ffnn* h);
/* feats [T x in0]; scores [T x out_last] = -(W x + b - alpha * log_prior) */
int amx_ffnn_score(amx_ffnn* h, const float* feats_host, int T, float* scores_host);
int amx_ffnn_score_dev(amx_ffnn* h, const float* feats_dev, int feats_stride, int T, float* scores_dev);
/* Waits for everything enqueued on the handle's stream and reports the state of the passes so far: AMX_OK, or AMX_ERR_STATE if a pass
 * of an AMX_PREC_F16MX handle met a value outside the f16 range (the scores of that pass are not valid).  The other precisions have
 * no failing pass: for them this is amx_synchronize. */
int amx_ffnn_wait_dev(amx_ffnn* h);
/* The AMX_PREC_* the handle computes in, and (nullable) the statistic that decided it.  A scorer requested as AMX_PREC_F16MX whose
 * weights are heavy-tailed computes in AMX_PREC_BF16X3 instead: with one exponent per 32 k a block whose maximum dwarfs the rest loses
 * the fp6 image of the small values (error 54-115 x that of f32 accumulation instead of 27 x; profiles/r05/f16mx_families.log).
 * *mx_block_ratio = rms of the block maxima / rms of the elements, the largest over the layers: 2.4 for Gaussian weights, 3.0 Laplace,
 * 3.3 Student-t(4), 5.0 log-normal(1.5), 5.66 at most; the switch happens above 4.0 (amx_ffnn_model.tuning mx_fallback=off keeps
 * f16mx, =auto is the default). */
int amx_ffnn_precision(const amx_ffnn* h, double* mx_block_ratio);
/* Nn::NeuralNetworkForwardNode ("neural-network-forward", Nn/Module.cc:107, Nn/NeuralNetworkForwardNode.cc:140-180): the network's
 * top-layer output per frame instead of a score.  AMX_NN_TOP_LINEAR: W x + b - alpha * log_prior (what a linear+softmax layer
 * yields with evaluate-softmax = false; exactly -score).  AMX_NN_TOP_SOFTMAX: the layer's default -- Math::FastMatrix<f32>::softmax
 * per frame (maximum, exp of the difference as ::exp(double) narrowed, sequential f32 sum, times (f32)1 / sum).  out [T x out_last]
 * in the network's own output order: a handle created with class_to_output is refused. */
enum { AMX_NN_TOP_LINEAR = 0, AMX_NN_TOP_SOFTMAX = 1 };
int amx_ffnn_forward_dev(amx_ffnn* h, const float* feats_dev, int feats_stride, int T, float* out_dev, int top);
/* Same, and additionally the per-epoch statistics of amx_stats_accumulate_dev for these frames: the arg-min over
 * the states is taken in the output layer's epilogue, so the [T x n_states] score matrix is written once and
 * never re-read.  best_state_dev nullable [T]. */
int amx_ffnn_score_stats_dev(amx_ffnn* h, const float* feats_dev, int feats_stride, int T, float* scores_dev,
                             uint32_t* best_state_dev, unsigned long long* state_counts_dev, double* score_sum_dev);

/* Nn::OnDemandFeatureScorer (Nn/FeatureScorer.cc:37-135): the hidden layers run once per frame
 * (forwardHiddenLayers), the output layer is evaluated only for the emissions the decoder asks for
 * (LinearAndSoftmaxLayer::getScore, Nn/LinearAndActivationLayer.cc:154-160: -bias[e] - W[e] . activation).
 * act_dev [T x amx_ffnn_hidden_dim] f32; pairs (frame_dev[p], emission_dev[p]) -> scores_dev[p]. */
int amx_ffnn_hidden_dim(const amx_ffnn* h);
int amx_ffnn_forward_hidden_dev(amx_ffnn* h, const float* feats_dev, int feats_stride, int T, float* act_dev);
int amx_ffnn_score_on_demand_dev(amx_ffnn* h, const float* act_dev, int n_pairs, const uint32_t* frame_dev, const uint32_t* emission_dev,
                                 float* scores_dev);
/* Nn::PrecomputedFeatureScorer (Nn/FeatureScorer.cc:291-310): the features are network outputs computed elsewhere;
 * score(e) = -x[out(e)] + alpha * logPrior[out(e)], Core::Type<f32>::max for a disregarded class.
 * class_to_output_dev nullable (identity); log_prior_dev indexed by network output. */
int amx_precomputed_score_dev(amx_ctx* ctx, const float* feats_dev, int feats_stride, int T, int n_classes, const int* class_to_output_dev,
                              const float* log_prior_dev, float prior_scale, float* scores_dev);

/* Nn::ClassLabelWrapper::initMapping (Nn/ClassLabelWrapper.cc:56-70): classes listed in `disregard` map to -1, the others to
 * consecutive network outputs.  mapping [n_classes]; *n_targets = classes to accumulate. */
int amx_class_labels_init(int n_classes, const int* disregard, int n_disregard, int* mapping, int* n_targets);
/* Math::Vector<T> files as Math::Module's format set reads and writes them (Math/Module.cc:25-41, Core/VectorParser.hh,
 * Math/Vector.hh:286-290,357-367): XML `<vector-f32 size="n"> v ... </vector-f32>` by default, `bin:<path>` = u32 n + raw
 * elements (f32 only; the reference registers no binary format for s32).  Nn::Prior::read / write (Nn/Prior.cc:211-245) use the
 * f32 form, ClassLabelWrapper::load / save (Nn/ClassLabelWrapper.cc:72-96) the s32 form.  *data is malloc'ed (amx_free). */
int amx_nn_vector_read_f32(const char* path, int* n, float** data);
int amx_nn_vector_write_f32(const char* path, int n, const float* data);
int amx_nn_vector_read_s32(const char* path, int* n, int** data);
int amx_nn_vector_write_s32(const char* path, int n, const int* data);
/* Math::Vector<u32> (maxoutvar's `maxout-sizes`): XML `<vector-u32 size="n">` or `bin:<path>` (u32 n + raw elements; Math/Module.cc:28-29
 * registers both for u32).  A file of another element type is refused.  *data is malloc'ed (amx_free). */
int amx_nn_vector_read_u32(const char* path, int* n, uint32_t** data);

/* ------------------------------------------------------------------ device buffers for resident score blocks
 * A decoder asks for ONE score at a time (Mm::FeatureScorer::ContextScorer::score, Mm/FeatureScorer.hh:31-46) and usually for a few
 * hundred of the 10^4 emissions of a frame; copying every [bufferSize x nEmissions] block to the host (40 kB per frame) would bound
 * the scorer at the PCIe rate.  These calls let a C / C++ adapter keep the block in HBM (*_score_dev) and move only what is asked
 * for: whole rows (amx_copy_to_host of one row) or (row, emission) pairs (amx_gather_scores: device gather + one small copy).
 * amx_copy_to_device returns when the source buffer may be reused (a pageable source is staged by the runtime; for a pinned source the
 * copy is waited for); amx_copy_to_host / amx_gather_scores synchronise the stream.  amx_gather_scores checks every (row, column)
 * pair against the block's shape [n_rows x ld] and refuses the call (AMX_ERR_INVALID) if one lies outside. */
int  amx_device_malloc(amx_ctx* ctx, size_t bytes, void** dev);
void amx_device_free(amx_ctx* ctx, void* dev);
int  amx_copy_to_device(amx_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  amx_copy_to_host(amx_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int  amx_gather_scores(amx_ctx* ctx, const float* scores_dev, int n_rows, int ld, int n, const uint32_t* rows_host,
                       const uint32_t* cols_host, float* dst_host);
/* Measurement: out_dev[0] = s_memtime (shader clock ticks), out_dev[1] = s_memrealtime (100 MHz), sampled by a one-wave kernel in stream
 * order.  Two samples around a stretch of work give the shader clock the chip sustained over it (delta ticks / delta 10 ns units); the
 * epoch run of bench.py prints it next to the real-time factor (Speech/CorpusProcessor.cc:49-58: wall time / audio time). */
int  amx_device_clocks_dev(amx_ctx* ctx, unsigned long long* out_dev);
/* The same per XCD: out_dev[2 x] / [2 x + 1] = (s_memtime, s_memrealtime) sampled on XCD x (eight one-wave workgroups, each filed under the
 * XCC id it reads; out_dev holds 16 values, zeroed by the caller -- an XCD no workgroup reached keeps its zeros).  The eight XCDs are
 * clocked separately.  s_memtime counts per CU and the CUs' counters are not aligned with one another: a difference of two samples is off by
 * the offset of the two CUs that took them (milliseconds' worth of ticks) -- meaningful over seconds (bench.py's full-epoch line), not over
 * one pass; s_memrealtime is one counter for the chip. */
int  amx_device_clocks_xcd_dev(amx_ctx* ctx, unsigned long long* out_dev);

/* ------------------------------------------------------------------ feature caches */

/* Core::FileArchive, the single-file "SP_ARC1" container RASR keeps feature caches, alignments and lattices in
 * (src/Core/FileArchive.cc:27-85 format, :165-225 open, :300-458 table / scan, :504-563 write; compression
 * src/Core/Archive.cc:52-222).  Host-side IO, no device involved.  AMX_ARCHIVE_WRITE opens read-write and creates the
 * file if it is missing or empty; an existing entry of the same name is replaced (the reference's
 * allow-overwrite=true).  amx_archive_close writes the file-info table (FileArchive::~FileArchive); an archive that
 * was never closed is still readable through the recovery-tag scan.  Directory and bundle archives are not handled. */
typedef struct amx_archive amx_archive;
#define AMX_ARCHIVE_READ 0
#define AMX_ARCHIVE_WRITE 1
int amx_archive_open(const char* path, int mode, amx_archive** out);
int amx_archive_close(amx_archive* a);
int amx_archive_n_files(amx_archive* a);
/* i-th live entry in archive order; *name stays valid until the archive is modified or closed. */
int amx_archive_file_info(amx_archive* a, int i, const char** name, uint32_t* size, uint32_t* compressed);
int amx_archive_has_file(amx_archive* a, const char* name);
/* Archive::readFile: *data is the uncompressed content, malloc'ed (amx_free). */
int amx_archive_read_file(amx_archive* a, const char* name, void** data, size_t* len);
/* Archive::writeFile: compress != 0 stores the gzip member the reference assembles (Archive.cc:162-215). */
int amx_archive_write_file(amx_archive* a, const char* name, const void* data, size_t len, int compress);
int amx_archive_remove_file(amx_archive* a, const char* name);

/* One Flow cache entry (= one segment) of vector-f32 packets, as Flow::CacheWriter / CacheReader exchange them
 * (src/Flow/Cache.cc:47-120, src/Flow/Datatype.cc:28-52, src/Flow/Vector.hh:88-106): blocks of
 * [string "vector-f32"][u32 n][n x (u32 dim, f32 x dim, f64 start, f64 end)].
 * feats [n x dim] row-major, times [n x 2] (start, end) -- the layout amx_gmm_score / amx_ffnn_score take.
 * gather: the node's `gather` parameter (a block holds gather+1 packets; 0xffffffff = one block per segment).
 * read: *feats / *times are malloc'ed (amx_free), times nullable; entries holding another datatype or vectors of
 * differing size return AMX_ERR_UNSUPPORTED. */
int amx_feature_cache_write(amx_archive* a, const char* segment, int n, int dim, const float* feats, const double* times,
                            unsigned gather, int compress);
int amx_feature_cache_read(amx_archive* a, const char* segment, int* n, int* dim, float** feats, double** times);
/* "<segment>.attribs": the Flow::Attributes of the cached stream as the reference's XmlWriter prints them
 * (src/Flow/Cache.cc:78-85, src/Flow/Attributes.hh:67-70,132-138).  read returns the XML text (amx_free). */
int amx_feature_cache_write_attributes(amx_archive* a, const char* segment, int n, const char* const* names,
                                       const char* const* values, int compress);
int amx_feature_cache_read_attributes(amx_archive* a, const char* segment, char** xml);

/* ------------------------------------------------------------------ NN parameter files and the state prior */

/* Binary Math::Matrix<f32> as RASR writes NN layer parameters ("bin:<base>-f32-layer-<i>.bin",
 * Nn/NeuralNetwork.cc:542-570; layout Math/Matrix.hh:560-574 + Math/Vector.hh:286-299): u32 rows, u32 cols, u32 rows,
 * then per row u32 cols + f32 values.  *data is malloc'ed row-major [rows x cols]; release it with amx_free. */
int  amx_nn_matrix_read(const char* path, int* rows, int* cols, float** data);
int  amx_nn_matrix_write(const char* path, int rows, int cols, const float* data);
void amx_free(void* p);
/* LinearLayer::setParameters (Nn/LinearLayer.cc:383-420): parameter matrix [out x (has_bias + in)], column 0 = bias,
 * -> W [out x in] row-major (== weights_[0] [in x out] column-major) and bias [out] (nullable). */
int amx_nn_layer_from_parameters(const float* params, int rows, int cols, int has_bias, float* W, float* bias);
/* Nn::Prior<f32>::setFromMixtureSet (Nn/Prior.cc:159-188), one-to-one class mapping: log_prior [n_mix]. */
int amx_prior_from_mixture_set(const amx_gmm_model* model, float* log_prior);

/* ------------------------------------------------------------------ per-epoch statistics */

/* For every frame t: best state = argmin_e scores[t][e] (first minimum wins);
 * state_counts[e] += 1 (u64), *score_sum += scores[t][best] (f64).  The caller all-reduces
 * state_counts / score_sum across ranks once per epoch. best_state_dev nullable [T]. */
int amx_stats_accumulate_dev(amx_ctx* ctx, const float* scores_dev, int T, int n_emissions,
                             uint32_t* best_state_dev, unsigned long long* state_counts_dev,
                             double* score_sum_dev);

/* ------------------------------------------------------------------ the per-epoch exchange between data-parallel ranks
 * The reference has no communication layer: `acoustic-model-trainer` processes take `partition = N`, `select-partition = k`
 * (segment i belongs to process i % N, src/Bliss/CorpusDescription.cc:174-190), write one accumulator file each, and
 * `combine-mixture-set-estimators` adds the files up offline (src/Tools/AcousticModelTrainer/AcousticModelTrainer.cc:317-325 ->
 * src/Mm/AbstractMixtureSetEstimator.cc:173-250).  Here the ranks of one node (one process and one amx_ctx per GPU) keep their
 * accumulators resident in HBM -- ONE flat f64 buffer per rank: amx_gmm_accumulator_size() doubles of statistics, score sums, and
 * the u64 counters converted with amx_counts_to_f64_dev -- and add them with ONE RCCL all-reduce over xGMI per epoch.
 *
 *   rank 0:  amx_comm_unique_id(id);  hand the 128 bytes to the other ranks (file, environment, MPI, socket: the caller's business)
 *   all:     amx_comm_init(ctx, rank, world, id, &comm);          collective: returns when all `world` ranks have called it
 *            ... one epoch of amx_*_score_stats_dev / amx_gmm_accumulate_dev into the flat buffer ...
 *            amx_comm_all_reduce_f64_dev(comm, flat_dev, n);      in place, on the context's stream, sum over ranks
 *
 * RCCL is bound at run time (dlopen of librccl.so; AMX_RCCL_LIB names another file): the library loads and every other entry
 * point works without it, amx_comm_available() tells.  The result equals the single-process accumulators up to the f64 summation
 * order of the ring.  A communicator belongs to its context (same device, same stream) and must be destroyed before it. */
typedef struct amx_comm amx_comm;
#define AMX_COMM_ID_BYTES 128
int  amx_comm_available(void);
int  amx_comm_unique_id(unsigned char id[AMX_COMM_ID_BYTES]);
int  amx_comm_init(amx_ctx* ctx, int rank, int world, const unsigned char id[AMX_COMM_ID_BYTES], amx_comm** out);
int  amx_comm_rank(const amx_comm* c);
int  amx_comm_world(const amx_comm* c);
int  amx_comm_all_reduce_f64_dev(amx_comm* c, double* buf_dev, size_t n);
void amx_comm_destroy(amx_comm* c);
/* Integer counters (state counts: u64, Mm/AbstractMixtureSetEstimator.cc keeps them as Weight = f64 anyway) ride in the same f64
 * buffer: exact below 2^53.  counts -> doubles before the all-reduce, doubles -> counts (rounded to nearest) after it. */
int amx_counts_to_f64_dev(amx_ctx* ctx, const unsigned long long* counts_dev, double* out_dev, size_t n);
int amx_f64_to_counts_dev(amx_ctx* ctx, const double* in_dev, unsigned long long* counts_dev, size_t n);

/* ------------------------------------------------------------------ NN training statistics
 * Nn::FeedForwardTrainer in batch mode (`estimator = dummy | dry-run`, the estimators the reference ships): forward, cross-entropy
 * error signal from the aligned labels, error backpropagation, per-layer gradient sums -- the pass that writes an Nn::Statistics
 * file for BatchEstimator -- and Nn::MeanAndVarianceTrainer's feature sums.  The update step and the regulariser: "NN mini-batch training" below.
 *
 * Per call of amx_nntrain_accumulate_dev (one mini-batch of the reference: Nn/FeedForwardTrainer.cc:215-269 processBatch_feedInput,
 * :401-443 finishWithAlignment, :272-337 finishWithError in batch mode), for frame t with class e = emission_dev[t]:
 *   output o = class_to_output[e]; a disregarded class (-1) never enters the batch (Nn/BufferedAlignedFeatureProcessor.cc:133-145):
 *       the frame adds to nothing, observations included;
 *   weight w = class_weights[o] (f32), then *= weight_dev[t] (f64), narrowed (:209-221); totalWeight += |w| (weights->asum());
 *   CLASS_COUNTS        count[o] += 1 (Nn/FeedForwardTrainer.cc:525-529);
 *   MEAN_AND_VARIANCE   sum += x * w, sumOfSquares += (x * x) * w on the RAW features, each product rounded to f32
 *                       (Nn/NeuralNetworkTrainer.cc:465-493);
 *   BASE                p = softmax of the top layer as amx_ffnn_forward_dev(..., AMX_NN_TOP_SOFTMAX) defines it; errors += (argMax(p)
 *                       != o) with argMax = the first strictly greater value from the start value Core::Type<f32>::min
 *                       (Math/FastMatrix.hh:899-909,1089-1101: a NaN never wins, a frame of -max/-inf/NaN only answers 0); objective
 *                       += -(logf(p[o])) * w, the term in f32 (Nn/Criterion.cc:55-69, Math/FastMatrix.hh:1105-1130: std::log on a
 *                       float); a p[o] that underflowed to 0 makes the objective +inf, and it is kept so, as the reference keeps it;
 *   GRADIENT            E_top = (p - delta_o) * w (Nn/Criterion.cc:77-98, Math/FastMatrix.hh:1061-1070: p + (-1), then scal by w);
 *                       for l = top .. 1: E_l is clipped to +-error_signal_clip (Nn/FeedForwardTrainer.cc:479-497,
 *                       Math/FastMatrix.hh:1306-1311; not the lowest layer), E_{l-1} = (W_l^T E_l) (.) f'(Y_{l-1})
 *                       (Nn/LinearLayer.cc:325-367; Math/FastMatrix.hh:1019-1057: sigmoid  e = (f32)((f64)e * ((f64)y * (1.0 - y))),
 *                       tanh  e = (f32)((f64)e * (1.0 - (f64)(y * y))) with y * y an f32 product, rectified  e = 0 where y <= 0);
 *                       G_l += X_l E_l^T, g_l += sum_t E_l[:, t] (:500-522), X_0 = the features behind the preprocessing layers.
 *
 * The accumulator is ONE caller-owned flat f64 device buffer of amx_nntrain_accumulator_size() doubles, zeroed by the caller, like
 * amx_gmm_accumulator_size()'s: ranks combine it with amx_comm_all_reduce_f64_dev.  amx_nntrain_layout() gives the offset of every
 * block; a block whose AMX_NNSTAT_* bit is not set has offset -1 and takes no room:
 *   per layer: gradient [in x out] row-major (the order of the file's Math::Matrix), then the bias gradient [out]     (GRADIENT)
 *   feature sum [feature_dim], sum of squares [feature_dim]                                                           (MEAN_AND_VARIANCE)
 *   class counts [n_outputs], one per network output                                                                  (CLASS_COUNTS)
 *   tail: nObservations, nClassificationErrors, totalWeight, objective (always; integers ride as f64, exact below 2^53)
 * This is the reference's `double-precision-accumulator = true`: a call's gradient is formed in f32 from zero, widened and added
 * (Nn/FeedForwardTrainer.cc:351-352, Nn/Statistics.hh:272-309), and the file narrows to f32 as finalize() does (:150-173).
 * Summing across calls in f32 (the reference's other mode) is not offered.
 *
 * Order of every sum: fixed by the call alone (the frames, T, the network), never by tile choice, occupancy or earlier calls.  Frames
 * are cut into chunks of AMX_NNTRAIN_CHUNK; within a chunk an element of X E^T, of the bias gradient and of the feature sums is one
 * ascending-t f32 chain, the chunk partials are added in f32 in ascending order, and the total is widened into the buffer.  Objective
 * terms are summed in f64.  The same call gives the same bits.
 *
 * Labels are checked on the device before anything is written: emission_dev[t] >= n_classes, or an output index >= n_outputs, makes
 * the call return AMX_ERR_INVALID naming the first such frame (the reference `require`s), acc_dev untouched; a bad label never
 * becomes an address.  At most AMX_NNTRAIN_MAX_FRAMES frames per call (split longer batches: the buffer adds up).  The cap bounds the
 * handle's workspace: besides every layer's input and error signal [T x units] it keeps the chunk partials of the largest layer,
 * ceil(T / AMX_NNTRAIN_CHUNK) x in x out f32 (padded to 128): 0.33 GB at T = 1024 and 1.3 GB at T = 4096 for a 2048 -> 10000 output layer.
 *
 * model: the struct the scorers take; precision must be AMX_PREC_FP32, log_prior / prior_scale are not read (a training network has
 * no prior), the last layer is linear with the softmax on top.  Hidden activations NONE, RELU, SIGMOID, TANH; preprocessing layers of
 * amx_ffnn_layers run first and are not trainable.  AMX_ERR_UNSUPPORTED with a message naming the layer: ELU, maxout, any other
 * precision.  Every layer is trained: amx_ffnn_model has no per-layer `trainable` switch, so a network with a frozen layer cannot be
 * described and gets a gradient block for that layer too (the caller ignores it).  model == NULL is allowed when the mask has neither BASE nor GRADIENT (MeanAndVarianceTrainer needs no network): the
 * dimensions then come from cfg.feature_dim and cfg.n_outputs. */
typedef struct amx_nntrain amx_nntrain;
enum { AMX_NNSTAT_CLASS_COUNTS = 1, AMX_NNSTAT_MEAN_AND_VARIANCE = 2, AMX_NNSTAT_BASE = 4, AMX_NNSTAT_GRADIENT = 8 };
#define AMX_NNTRAIN_CHUNK 256
#define AMX_NNTRAIN_MAX_FRAMES 4096
#define AMX_NNTRAIN_MAX_LAYERS 16
typedef struct {
    int          statistics;        /* AMX_NNSTAT_* mask (default BASE | GRADIENT) */
    float        error_signal_clip; /* `error-signal-clip`; Core::Type<f32>::max = off (default) */
    const float* class_weights;     /* nullable [n_outputs] (`class-weights-file`); NULL = 1 */
    int          feature_dim;       /* model == NULL only: the feature dimension */
    int          n_outputs;         /* model == NULL only: the number of network outputs (class counts) */
    int          n_classes;         /* model == NULL only: length of class_to_output (ignored when that is NULL) */
    const int*   class_to_output;   /* model == NULL only: as amx_ffnn_model.class_to_output, nullable */
} amx_nntrain_cfg;
typedef struct {
    int  n_layers, feature_dim, n_outputs;
    int  in_dim[AMX_NNTRAIN_MAX_LAYERS], out_dim[AMX_NNTRAIN_MAX_LAYERS];
    long gradient_weights[AMX_NNTRAIN_MAX_LAYERS], gradient_bias[AMX_NNTRAIN_MAX_LAYERS]; /* offsets in doubles, -1 = absent */
    long feature_sum, feature_square_sum, class_counts;
    long tail; /* nObservations, nClassificationErrors, totalWeight, objective */
    long size;
} amx_nntrain_layout_info;
void amx_nntrain_default_cfg(amx_nntrain_cfg* cfg);
/* ctx == NULL gives a host-only handle (layout, files, prior, mean and deviation); amx_nntrain_accumulate_dev on it is AMX_ERR_STATE */
int  amx_nntrain_create(amx_ctx* ctx, const amx_ffnn_model* model, const amx_ffnn_layers* layers, const amx_nntrain_cfg* cfg, amx_nntrain** out);
void amx_nntrain_destroy(amx_nntrain* h);
long amx_nntrain_accumulator_size(const amx_nntrain* h);
int  amx_nntrain_layout(const amx_nntrain* h, amx_nntrain_layout_info* info);
/* feats_dev [T x feats_stride] f32, emission_dev [T] class indices (`emission_dev` of the aligners; nullable when the mask is
 * MEAN_AND_VARIANCE alone), weight_dev nullable [T] f64 alignment weights.  The call waits for the label check only. */
int  amx_nntrain_accumulate_dev(amx_nntrain* h, const float* feats_dev, int feats_stride, int T, const uint32_t* emission_dev,
                                const double* weight_dev, double* acc_dev);
/* Nn::Statistics<f32> files (Nn/Statistics.cc:345-389,584-604): 16-byte magic "NNSTAT" + C/# M/# B/# G/# + S + "#####", u32 version 2,
 * u32 nObservations, f32 totalWeight; BASE: u32 errors, f32 objective; CLASS_COUNTS: u32 n, then (class, count) pairs of the classes
 * seen, ascending; MEAN_AND_VARIANCE: two Math::Vector<f32> (u32 size, elements); GRADIENT: u32 nLayers, per layer u32 nStreams = 1,
 * Math::Matrix<f32> [in x out] (u32 rows, u32 columns, u32 rows, per row u32 columns + elements) and Math::Vector<f32> [out].
 * write narrows the f64 buffer to f32 (u32 for the integers).  read OVERWRITES acc_host with the file's values; the file's magic must
 * carry exactly the handle's mask, version 2 and the handle's shapes (AMX_ERR_INVALID), precision letter D is AMX_ERR_UNSUPPORTED.
 * combine (Nn/Statistics.cc:514-536, Nn/Statistics.hh:272-309): the first file read, the others added IN f32 in the order given, as
 * Statistics<f32>::combine does, then widened into acc_host. */
int  amx_nnstat_write(const amx_nntrain* h, const double* acc_host, const char* path);
int  amx_nnstat_read(const amx_nntrain* h, const char* path, double* acc_host);
int  amx_nnstat_combine(const amx_nntrain* h, const char* const* paths, int n, double* acc_host);
/* Nn::Prior::setFromClassCounts (Nn/Prior.cc:128-156): v = max(count, back-off count) as u32, as f32 times the class weight; log of
 * v / sum(v) (std::log on a float, the sum sequential in f32), Core::Type<f32>::min where v == 0.  log_prior [n_outputs].
 * back_off_count must be a whole number >= 0 (`back-off-count` is a u32 there).  Needs CLASS_COUNTS. */
int  amx_prior_from_class_counts(const amx_nntrain* h, const double* acc_host, float back_off_count, float* log_prior);
/* Nn::Statistics<f32>::finalize + MeanAndVarianceTrainer::writeMeanAndStandardDeviation (Nn/Statistics.cc:146-173,
 * Nn/NeuralNetworkTrainer.cc:447-462) on the narrowed sums: a = (f32)(1.0 / totalWeight); mean = sum * a; stddev = sqrt(sumOfSquares
 * * a + (-1 * (mean * mean))), every step in f32.  mean, stddev [feature_dim]: what `mean-and-variance-normalization` reads
 * (amx_nn_vector_write_f32).  Needs MEAN_AND_VARIANCE. */
int  amx_nnstat_mean_and_deviation(const amx_nntrain* h, const double* acc_host, float* mean, float* stddev);

/* ------------------------------------------------------------------ NN mini-batch training
 * Nn::FeedForwardTrainer with `batch-mode = false` on the handle above: what runs on every mini-batch besides the statistics pass --
 * the regulariser on the objective and on the gradient, Statistics::finalize, the estimator's step on the weights and
 * `accumulate-multiple-batches` -- and Nn::BatchEstimator on a combined statistics buffer.  The statistics of a group of mini-batches
 * are single precision and live in the handle, beside the weight image W [out x in] the forward GEMM reads and the transposed image
 * W^T [in x out] the backward GEMM reads; the step updates both images in one pass, nothing travels to the host.
 *
 * Per mini-batch (amx_nntrain_step_accumulate_dev), with A = accumulate_multiple_batches and n the running mini-batch count
 * (Nn/FeedForwardTrainer.cc:215-269,272-337):
 *   1. n += 1; if (n - 1) % A == 0 the group's statistics are reset (:235-238);
 *   2. observations, total weight, errors and the forward pass as amx_nntrain_accumulate_dev defines them; the objective of the call
 *      (its terms summed in f64, as there) is narrowed and added to the group's f32 objective;
 *   3. objective += regularizer.objectiveFunction(network, (f32)T) (:290-296, Nn/Regularizer.cc:74-94,129-149,182-212): over the
 *      trainable layers with regularization_constant c > 0, in f32,  tmp = norm(b); tmp += norm(W); tmp *= c (l1: norm = asum) or
 *      tmp = (f32)((f64)tmp * (c / 2.0)) (l2: norm = dot; centered-l2: of b - b_c, W - W_c); obj += tmp; the result T * obj.  T = the
 *      frames that entered the batch.  norm is a two-stage f64 sum in a fixed order (segments of 4096 elements of the padded image, the
 *      segment sums added by one workgroup), narrowed to f32 where asum / dot return;
 *   4. error backpropagation and the gradient as there; the call's total -- the same f32 bits that amx_nntrain_accumulate_dev widens
 *      -- is added to the group's statistic with one f32 add;
 *   5. regularizer.addGradient(network, statistics, (f32)nObservations) (:331-336, Nn/Regularizer.cc:97-119,152-165,215-234), per
 *      element one fused multiply-add as saxpy computes it:  G = fmaf(c * factor, W, G) (l2), fmaf(c * factor, sign(W), G) (l1),
 *      fmaf(c * factor, W, G) then fmaf(-(c * factor), W_c, .) (centered-l2), the bias alike.  factor is the group's RUNNING number of
 *      observations, this call included, so with A > 1 it grows from call to call, as in the reference.  It is fused into the kernel
 *      that adds the call's gradient.
 * The step (amx_nntrain_step_estimate_dev; amx_nntrain_step_dev runs it when n % A == 0, :339-349):
 *   6. Statistics::finalize (Nn/Statistics.cc:146-161): with normalize_by_observations and nObservations != 1, every gradient element
 *      *= (f32)(1.0 / (f32)nObservations) (sscal: one product) and objective = (f32)((f64)objective * (1.0 / (f32)nObservations));
 *   7. the estimator, the text of Nn::MeanNormalizedSgd::estimate and MeanNormalizedSgdL1Clipping::estimate
 *      (Nn/MeanNormalizedSgdEstimator.cc:51-126,136-153).  Per trainable layer l, with m the activation mean of what feeds it when that
 *      keeps statistics (see below):  G[i][o] = fmaf(m[i], -g[o], G[i][o])  (addOuterProduct(m, g, -1): sger rounds alpha * y first);
 *      W = fmaf(-(eta * eta_l), G, W);  g[o] = g[o] - sum_i G[i][o] m[i]  (multiply(m, g, transposed, -1, 1): sgemv, the sum in the order
 *      given below);  b = fmaf(-((eta * eta_bias) * eta_l), g, b).  Without statistics the two terms with m are skipped.
 *      With log_step_size  step_l = (0 + asum(G) * (eta * eta_l)) + asum(g) * ((eta * eta_bias) * eta_l);  the l1-clipping estimator
 *      then moves every weight and bias towards zero by v = (c_l * eta) * eta_l (Math/FastMatrix.hh:1291-1303, Math/FastVector.hh:
 *      500-509:  w > 0: max(0, w - v),  w < 0: min(0, w + v),  a zero of either sign stays).  The gradient blocks hold the finalized
 *      gradient afterwards.  These two are the only update rules the reference's tree carries; its createEstimator
 *      (Nn/Estimator.cc:87-104) offers `dummy` and `dry-run` only, so the text defines the arithmetic, not a reachable configuration.
 *      update_input_layer_weights: the reference's loop over a layer's input streams runs to nPredecessors(), and a layer fed by the
 *      feature stream has none (Nn/NetworkTopology.cc:58-83, Nn/NeuralNetwork.cc:157-166), so as the text stands the first layer of a
 *      network without preprocessing layers gets its bias updated and its weights never (nor do they count in step_l).  1 (default)
 *      updates them like every other layer's; 0 gives the text as it stands.
 * Activation statistics (Nn/NeuralNetwork.cc:423, Nn/NeuralNetworkLayer.cc:189-334): after the forward pass of a mini-batch of T frames
 * that entered it, a layer whose smoothing is not no-statistics updates per output unit, y its output:
 *   none               sum += sum_t y,  sumSq += sum_t y * y,  nObs += T;
 *   exponential-trace  on its first batch sum = sum_t ((f32)1 / T) y and sumSq = sum_t (f32)(1.0 / T) y * y (each unless an initial mean
 *                      / deviation was given); then on every batch, the first included, sum = f * sum; sum += sum_t (((f32)1 - f) / T) y,
 *                      sumSq alike; nObs counts as 1.
 *   initial mean and deviation (`old-activations-*-file`): on the first batch nObs = 1 (trace) or T, sum = mean * nObs,
 *                      sumSq = (dev * dev + mean * mean) * nObs, every step in f32.
 *   mean = fmaf((f32)(1.0 / nObs), sum, 0);  variance = fmaf((f32)(1.0 / nObs), sumSq, -1 * (mean * mean)), then * 1 and + 0
 *   (`activation-variance-interpolation` is 1, its default).
 * The sums are the loops  at(row) += scale * m  and  at(row) += scale * m * m  of Math/FastVector.hh:461-478, contraction sites of the
 * reference's default build: with amx_set_contract(AMX_CONTRACT_FMA) acc = fmaf(scale, y, acc) and acc = fmaf(scale * y, y, acc), with
 * AMX_CONTRACT_OFF acc + scale * y and acc + (scale * y) * y; scale * y is rounded in both.  Order: frames ascending; the chain of the
 * call's first AMX_NNTRAIN_CHUNK frames starts from the value the sum holds (the reference's own chain for a mini-batch of up to 256
 * frames), every further chunk's chain starts from zero and the chunk totals are added in ascending order.
 * The output layer keeps no statistics (nothing reads them).  The layer that feeds layer 0 is the last preprocessing layer, when there
 * is one: input_smoothing.
 * sum_i G[i][o] m[i]: per 32-row tile one ascending chain of fused multiply-adds from zero, the tile totals added in ascending order.
 *
 * asum(G), asum(g): the 32 x 32 tiles of the update kernel sum |G| in f32 in a fixed order, the tile sums are added in f64 by one
 * workgroup in an order the layer's shape fixes, narrowed to f32.  No float atomics anywhere: the same calls give the same bits.
 *
 * amx_nntrain_estimate is Nn::BatchEstimator (Nn/BatchEstimator.cc:50-101) on a flat f64 buffer of this handle's layout
 * (amx_nnstat_read / amx_nnstat_combine, or an all-reduced acc_dev copied out): the buffer narrowed to f32 as the file narrows it
 * becomes the group's statistics, then the regulariser's objective and gradient with factor = nObservations, finalize, the estimator. */
enum { AMX_NNSTEP_REG_NONE = 0, AMX_NNSTEP_REG_L1 = 1, AMX_NNSTEP_REG_L2 = 2, AMX_NNSTEP_REG_CENTERED_L2 = 3 };
enum { AMX_NNSTEP_STAT_NO_STATISTICS = 0, AMX_NNSTEP_STAT_NONE = 1, AMX_NNSTEP_STAT_EXPONENTIAL_TRACE = 2 };
enum { AMX_NNSTEP_MEAN_NORMALIZED_SGD = 0, AMX_NNSTEP_MEAN_NORMALIZED_SGD_L1_CLIPPING = 1 };
typedef struct {
    float               learning_rate;               /* `initial-learning-rate` (default 1) */
    float               bias_learning_rate;          /* `bias-learning-rate` (default 1) */
    const float*        layer_learning_rate;         /* nullable [n_layers] (`learning-rate` of a layer); NULL = 1 */
    const float*        regularization_constant;     /* nullable [n_layers] (`regularization-constant`); NULL = 0 */
    const int*          trainable;                   /* nullable [n_layers] (`trainable`); NULL = every layer */
    int                 regularizer;                 /* AMX_NNSTEP_REG_* (default none) */
    const float* const* center_W;                    /* centered-l2: [n_layers] of [out x in], the layout of amx_ffnn_model.W */
    const float* const* center_bias;                 /* centered-l2: [n_layers] of [out] */
    const int*          center_in_dim;               /* centered-l2: [n_layers], the centre's shapes (checked against the network's) */
    const int*          center_out_dim;
    int                 estimator;                   /* AMX_NNSTEP_MEAN_NORMALIZED_SGD* (default the plain one) */
    int                 accumulate_multiple_batches; /* A >= 1 (default 1) */
    int                 normalize_by_observations;   /* `normalize-by-num-observations` (default 1) */
    int                 log_step_size;               /* `log-step-size`: fill amx_nnstep_info.step_size (default 0) */
    int                 update_input_layer_weights;  /* see above (default 1) */
    const int*          statistics_smoothing;        /* nullable [n_layers] AMX_NNSTEP_STAT_* of each layer's output; NULL = no-statistics */
    const float*        trace_factor;                /* nullable [n_layers] `exponential-trace-interpolation-factor`; NULL = 0.5 */
    const float* const* initial_activation_mean;     /* nullable [n_layers] of nullable [out]: `old-activations-mean-file` */
    const float* const* initial_activation_stddev;   /* the same for `old-activations-standard-deviation-file`; given together with the mean */
    int                 input_smoothing;             /* AMX_NNSTEP_STAT_* of the last preprocessing layer; must be 0 without one */
    float               input_trace_factor;          /* default 0.5 */
    const float*        input_initial_mean;          /* nullable [feature_dim] */
    const float*        input_initial_stddev;
} amx_nnstep_cfg;
typedef struct {
    long  minibatch;               /* n: step_accumulate calls since amx_nntrain_set_estimator */
    int   updated;                 /* 1 when the group was finalized and the estimator ran */
    long  n_observations;          /* of the current group */
    long  n_classification_errors;
    float total_weight;
    float objective;               /* criterion + regulariser, the reference's objectiveFunction_; finalized when updated */
    float criterion_objective;     /* the same chain without the regulariser's terms */
    float step_size[AMX_NNTRAIN_MAX_LAYERS]; /* log_step_size and updated: step_l; 0 otherwise */
} amx_nnstep_info;
void amx_nnstep_default_cfg(amx_nnstep_cfg* cfg);
/* Needs a handle with a network whose statistics are exactly BASE | GRADIENT.  Copies what cfg points to, allocates the group's f32
 * statistics and the centre images, and resets the mini-batch counter; may be called again.  AMX_ERR_INVALID with a message naming the
 * field or the layer: a regularization constant < 0, A < 1, a learning rate that is not finite, a centre that is missing or of another
 * shape, no network.  A host-only handle takes the configuration (and its refusals) but cannot step. */
int  amx_nntrain_set_estimator(amx_nntrain* h, const amx_nnstep_cfg* cfg);
/* steps 1-5; arguments as amx_nntrain_accumulate_dev's, 1 <= T.  AMX_ERR_STATE on a host-only handle or before set_estimator */
int  amx_nntrain_step_accumulate_dev(amx_nntrain* h, const float* feats_dev, int feats_stride, int T, const uint32_t* emission_dev,
                                     const double* weight_dev);
/* steps 6-7 on the current group, whatever the counter says */
int  amx_nntrain_step_estimate_dev(amx_nntrain* h);
/* the two together under the counter rule; info nullable.  Filling info costs one small device-to-host copy at the end of the call,
 * besides the wait for the label check that every pass has. */
int  amx_nntrain_step_dev(amx_nntrain* h, const float* feats_dev, int feats_stride, int T, const uint32_t* emission_dev,
                          const double* weight_dev, amx_nnstep_info* info);
/* the current group as amx_nntrain_step_dev reports it (waits for the stream) */
int  amx_nntrain_step_info(amx_nntrain* h, amx_nnstep_info* info);
/* Nn::BatchEstimator, see above.  acc_host: amx_nntrain_accumulator_size() doubles */
int  amx_nntrain_estimate(amx_nntrain* h, const double* acc_host, amx_nnstep_info* info);
/* Read-back (each waits for the stream).  image 0 = the forward image W, 1 = the transposed one, both returned as W [out x in] and
 * bias [out] (either nullable); a host-only handle returns what it was created with.  Step statistics: the group's gradient G [in x
 * out] (the order of the file's Math::Matrix) and bias gradient g [out], after the step the finalized gradient. */
int  amx_nntrain_get_parameters(amx_nntrain* h, int layer, int image, float* W, float* bias);
int  amx_nntrain_get_step_statistics(amx_nntrain* h, int layer, float* G, float* g);
/* getActivationMean / getActivationVariance of `layer`'s output, [out] each (either nullable); layer -1 = the last preprocessing layer
 * ([feature_dim]).  AMX_ERR_STATE when that layer keeps no statistics or has seen no mini-batch yet. */
int  amx_nntrain_get_activation_statistics(amx_nntrain* h, int layer, float* mean, float* variance);
/* the input of `layer` (= the output of what feeds it) as the last pass left it: X [T x in], rows of frames that did not enter the
 * batch included (their inputs were packed as zeros).  T <= the frames of that pass. */
int  amx_nntrain_get_layer_input(amx_nntrain* h, int layer, int T, float* X);

/* ------------------------------------------------------------------ constrained MLLR (CMLLR), one affine feature transform per key */

/* Speech::AffineFeatureTransformEstimator over Mm::AffineFeatureTransformAccumulator (Mm/AffineFeatureTransformAccumulator.cc): the
 * corpus pass on the device (cmllr.hip), files / combine / estimate / score on the host (cmllr_host.cpp, no device needed), and the
 * application of the transforms with the key chosen per segment.  Criteria naive and mmi-prime; hlda is refused.
 *
 * A handle is created on an amx_gmm handle, which supplies means, diagonal variances, the density -> (mean, covariance) indices and
 * nCovariances.  feature_dim F is the width of the accumulated stream, model_dim M the model's dimension; F >= M (F < M is refused),
 * F <= 255, n_keys <= 65535 (a key is one row of the kernels' grid; AMX_ERR_UNSUPPORTED beyond), at most 2^30 frames per call.  The gmm
 * handle must outlive the cmllr handle.
 *
 * The accumulator is ONE flat f64 buffer the caller owns and zeroes, amx_cmllr_accumulator_size(h) doubles; per key, with R = F + 1
 * and `tri` = R (R + 1) / 2 the row-major UPPER triangle (j <= k) of an R x R matrix:
 *     [beta | k: M x R | mean: R | cov: tri | G: M x tri]
 * G only when the model has more than one covariance (amx_cmllr_shape.pooled == 0); a pooled model keeps its variance vector and
 * finalize derives G from cov (:124-133).  Ranks combine the buffer with amx_comm_all_reduce_f64_dev.
 *
 * Arithmetic of one frame x (f32, xi = [1, x] widened to f64) aligned to density d with mean m, variance v (f32, widened), :40-121:
 *     beta += 1 | w;  k[i][j] += m_i / v_i * xi_j [* w];  mean[j] += xi_j [* w];  cov[j][k] += xi_j * xi_k [* w];
 *     G[i][j][k] += xi_j * xi_k / v_i [* w]           (left to right, the division is an IEEE division, no reciprocal)
 * amx_set_contract(AMX_CONTRACT_FMA) makes the last multiplication of each `+= a * b` one fused multiply-add with the addition, the
 * sites the reference's -march=native build contracts (tests/golden/ref_cmllr.npz holds both builds).  Per (key, cell) the sum is
 * ONE chain over the key's frames in ascending frame order that continues from the value in the buffer: no floating-point atomics,
 * nothing depends on the launch shape, and a corpus fed in order and cut into calls anywhere gives the same bits. */
typedef struct amx_cmllr amx_cmllr;
typedef struct {
    int feature_dim, model_dim, n_keys;
    int pooled;            /* 1: the model has ONE covariance, no G block */
} amx_cmllr_shape;
int  amx_cmllr_create(amx_gmm* gmm, int feature_dim, int n_keys, amx_cmllr** out);
void amx_cmllr_destroy(amx_cmllr* h);
/* shape (nullable) and, for a pooled model, the variance vector [model_dim] (nullable; untouched otherwise) */
int  amx_cmllr_describe(const amx_cmllr* h, amx_cmllr_shape* shape, float* pooled_variance);
long amx_cmllr_accumulator_size(const amx_cmllr* h);                 /* doubles, all keys; 0 for NULL */
long amx_cmllr_key_size(const amx_cmllr_shape* shape);               /* doubles of ONE key; 0 for a bad shape */
/* frames per LDS stage, cells of the triangle per workgroup and model components per workgroup of the G kernel (any pointer nullable) */
void amx_cmllr_kernel_shape(int* stage_frames, int* tile_cells, int* tile_components);
/* Kernel selection for A/B runs and tests: the G kernel with 16 (default) or 48 model components per workgroup and lane -- 48 is the shape
 * in which a lane keeps all accumulators of a 45-dimensional model.  Both give the same bits (tests/test_cmllr_gpu.py); DESIGN.md
 * section 4.18 has their times.  Any other value: AMX_ERR_INVALID. */
int  amx_cmllr_set_tile(amx_cmllr* h, int tile_components);
/* feats_dev [frame x feats_ld] (feats_ld >= F); segment s covers frames [frame_offsets[s], frame_offsets[s + 1]) and adds to key
 * seg_key[s] (both host arrays); emission_dev[t] int32 as the aligners leave it, -1 skips the frame; the density is
 * best_density_dev[t * best_density_ld + emission] or best_density_dev[t] when best_density_ld == 0 (amx_gmm_accumulate_dev's
 * convention); weight_dev nullable f64 (a weight of exactly 0 still adds its zeros, as the reference does).
 * Checked on the device BEFORE anything is written: an emission index outside the model other than -1, a density outside its
 * mixture, a non-finite feature or weight -- AMX_ERR_INVALID naming the first such frame, acc_dev untouched.  Refused on the host: a
 * key outside [0, n_keys), decreasing offsets, NULL buffers where there are frames.  Waits for the stream. */
int  amx_cmllr_accumulate_dev(amx_cmllr* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets, const int* seg_key,
                              const int32_t* emission_dev, const uint32_t* best_density_dev, int best_density_ld, const double* weight_dev,
                              double* acc_dev);
/* y = A_key [1, x] per frame without materialising [1, x]: transforms_dev [n_keys x M x (F + 1)] f32, has_transform [n_keys] (host;
 * 0: the key's segments get the identity rows y_i = x_i, what estimate's early return gives, and *n_identity_segments (nullable)
 * counts them).  The dot product is amx_matrix_multiply_dev's (k ascending from the offset column, fused under AMX_CONTRACT_FMA): the
 * result equals that entry point run per segment on the extended features in every bit.  Overlapping views are rejected. */
int  amx_cmllr_apply_dev(amx_ctx* ctx, const float* transforms_dev, const int* has_transform, int n_keys, int model_dim, int feature_dim,
                         const float* in_dev, int in_ld, int n_seg, const long* frame_offsets, const int* seg_key, float* out_dev, int out_ld,
                         int* n_identity_segments);

/* ---- host side (cmllr_host.cpp): `acc` is ONE key's part of the flat buffer, amx_cmllr_key_size(shape) doubles, host memory;
 * pooled_variance [M] f32 is read when shape->pooled (amx_cmllr_describe). */
/* The reference's binary accumulator behind Core::IoRef's type-name tag (Core/IoRef.hh:119-122, :367-377), little endian:
 *   u32 36 "affine-feature-transform-accumulator" | u32 F | u32 M | f64 beta | vector<Matrix<f64>> G | vector<Vector<f64>> k |
 *   Vector<f64> mean | Matrix<f64> cov | vector<f32> globalModelVariance | u8 globalVarianceOptimization (0xff | 0)
 * as the accumulating pass leaves it: upper triangles filled, lower ones zero; a pooled model's G matrices are 0 x 0.
 * read: the file's F, M and pooled flag must equal the shape's (and its variance vector pooled_variance); a wrong tag, a truncated
 * file or a G / cov with a non-zero lower triangle (a finalized accumulator) is AMX_ERR_INVALID. */
int  amx_cmllr_accumulator_write(const amx_cmllr_shape* shape, const float* pooled_variance, const double* acc, const char* path);
int  amx_cmllr_accumulator_read(const amx_cmllr_shape* shape, const float* pooled_variance, const char* path, double* acc);
/* combine (:345-365): acc += other * weight, member by member; its verify()s as errors (dimensions, pooled against non-pooled, unequal
 * variance vectors) */
int  amx_cmllr_combine(const amx_cmllr_shape* shape, const float* pooled_variance, double* acc, const amx_cmllr_shape* other_shape,
                       const float* other_variance, const double* other_acc, double weight);
enum { AMX_CMLLR_NAIVE = 0, AMX_CMLLR_MMI_PRIME = 1, AMX_CMLLR_HLDA = 2 };
/* finalize (:123-143) + estimate (:177-311), operation by operation in f64, the inverse by an LU with partial pivoting (the reference
 * calls dgetrf / dgetri; see DESIGN.md section 4.18 for the measured distance).  initial: nullable (identity, :169-174), M x
 * initial_cols with initial_cols == F (a zero column is put in front) or F + 1.  transform_out [M x (F + 1)] f32; transform64_out
 * (nullable) the same before the narrowing; iterations_out (nullable) [iterations x M x (F + 1)] f64 the transform after every
 * iteration (mmi-prime).  *estimated (nullable) = 0 when beta < min_obs_weight returned the initial transform (:204-205).
 * AMX_CMLLR_HLDA: AMX_ERR_UNSUPPORTED.  A singular G or pseudo-inverse: AMX_ERR_INVALID. */
int  amx_cmllr_estimate(const amx_cmllr_shape* shape, const float* pooled_variance, const double* acc, int iterations, double min_obs_weight,
                        int criterion, const float* initial, int initial_cols, float* transform_out, double* transform64_out,
                        double* iterations_out, int* estimated);
/* finalize + score (:313-343) of an M x (F + 1) f32 transform: jacobian - distance / beta */
int  amx_cmllr_score(const amx_cmllr_shape* shape, const float* pooled_variance, const double* acc, const float* transform, int criterion,
                     double* score_out);
/* The transform file the estimator writes per key (`os << transform` on a Core::XmlOutputStream, Speech/AffineFeatureTransformEstimator.cc:
 * 124-132; Math/Matrix.hh:641-647): the XML declaration, <matrix-f32 nRows nColumns>, one line per row with every value in scientific
 * notation with six digits and a space behind it, the closing tag -- byte for byte the reference's (tests/golden/ref_cmllr.npz).  A
 * non-finite element is refused.  read takes what an XML parser takes (declaration and comments in front, either quote, any white
 * space) and is also how an `initial-transform` is read; *data: rows x cols floats, amx_free(). */
int  amx_cmllr_transform_write(const char* path, int rows, int cols, const float* transform);
int  amx_cmllr_transform_read(const char* path, int* rows, int* cols, float** data);

/* ------------------------------------------------------------------ MLLR, mean transforms per key and regression class */

/* Speech::ModelTransformEstimator over Mm::FullAdaptorViterbiEstimator / Mm::ShiftAdaptorViterbiEstimator (Mm/MllrAdaptation.cc): the
 * corpus pass on the device (mllr.hip), files and the estimate on the host (mllr_host.cpp, no device needed), and the adapted mean
 * table of one key on the device.  Modes full and shift; band and semi-tied (MODULE_ADAPT_ADVANCED) are refused.
 *
 * A handle is created on an amx_gmm handle (which must outlive it).  leaf_of_mixture [n_mixtures] is the reference's leafIndex_ AS
 * MllrAdaptation.cc INDEXES IT, with the mixture index (Am/AdaptationTree.cc:95-99 appends the silence class), every value in
 * [0, n_leafs).  Limits: dimension D <= 255, n_keys <= 65535, n_leafs <= 4096 (the compaction kernel keeps a counter per leaf in
 * LDS; the reference's default is 70 + 1); AMX_ERR_UNSUPPORTED beyond, and for a model in which two (mixture, density) visits reach
 * the same mean (adaptMixtureSet would transform it twice, :147-148).  At most 2^30 frames per call.
 *
 * The accumulator is ONE flat f64 buffer the caller owns and zeroes, amx_mllr_accumulator_size(h) doubles, [key][leaf][cells]:
 *     full:   [count_Z | Z: D x (D + 1) | count_G | G: (D + 1) x (D + 1)]      (all of G, both triangles, both counts)
 *     shift:  [count | beta: D | shift: D]
 * Ranks may all-reduce the buffer (amx_comm_all_reduce_f64_dev); the reference has no combine for these classes
 * (AbstractAdaptationAccumulator::combine is defect()), so such sums are outside the bit-parity claim.
 *
 * Arithmetic of one frame x (f32) aligned to a density with mean m and variance v (f32), mt = [1, m] widened to f64:
 *     full (:599-653):   count_Z++, count_G++ (frames, also in the weighted overload);
 *                        Z[i][j] += x_i * mt_j           | (w * x_i) * mt_j
 *                        G[i][j] += mt_i * mt_j          | (w * mt_i) * mt_j
 *     shift (:381-416):  count += 1 | w;   beta[d] += 1.0 / v_d | w / v_d   (f64 divisions)
 *                        shift[d] += f64((x_d - m_d) / v_d)   (f32 subtraction and division)   |   w * f64(x_d - m_d) / v_d
 * The unweighted products are exact in f64, so both contract modes give the same bits; in the weighted full form
 * AMX_CONTRACT_FMA fuses Z's last product with the addition, as the reference's -march=native build does; that build leaves G's
 * product and addition apart, and so does the library in both modes (tests/golden/ref_mllr.npz holds both builds).  Per (key, leaf, cell) the sum is ONE chain over that key's frames of that leaf in
 * ascending frame order that continues from the value in the buffer: no floating-point atomics, no partial sums, nothing depends on
 * the launch shape, and a corpus fed in order and cut into calls anywhere gives the same bits. */
typedef struct amx_mllr amx_mllr;
enum { AMX_MLLR_FULL = 0, AMX_MLLR_SHIFT = 1, AMX_MLLR_BAND = 2, AMX_MLLR_SEMI_TIED = 3 };
typedef struct {
    int mode, dim, n_leafs, n_keys;
} amx_mllr_shape;
/* The pruned Core::BinaryTree (Core/BinaryTree.hh) over node ids 0 .. n_ids - 1, n_ids = numberOfNodes + numberOfLeafs: left / right
 * / previous per id (-1 = invalidId), leaf_number per id (-1 for an inner node), the leaf list as node ids in leafList() order, the
 * silence mixtures ascending (std::set order). */
typedef struct {
    int        n_ids, root;
    const int *left, *right, *previous, *leaf_number;
    int        n_leaf_list;
    const int* leaf_list;
    int        n_silence;
    const int* silence_mixtures;
} amx_mllr_tree;
int  amx_mllr_create(amx_gmm* gmm, int mode, int n_keys, int n_leafs, const int* leaf_of_mixture, amx_mllr** out);
void amx_mllr_destroy(amx_mllr* h);
int  amx_mllr_describe(const amx_mllr* h, amx_mllr_shape* shape);
long amx_mllr_accumulator_size(const amx_mllr* h);                  /* doubles, all keys; 0 for NULL */
long amx_mllr_leaf_size(const amx_mllr_shape* shape);               /* doubles of ONE (key, leaf); 0 for a bad shape */
long amx_mllr_key_size(const amx_mllr_shape* shape);                /* doubles of ONE key = n_leafs * leaf size */
/* frames per LDS stage and cells per workgroup of the accumulation kernel (any pointer nullable) */
void amx_mllr_kernel_shape(int* stage_frames, int* tile_cells);
/* Arguments and device checks as amx_cmllr_accumulate_dev: feats_dev [frame x feats_ld]; segment s covers frames [frame_offsets[s],
 * frame_offsets[s + 1]) of key seg_key[s]; emission_dev -1 skips the frame (the adapter sets it for alignment items below weight
 * 0.5, which accumulate(alignment, ...) of the shift estimator skips, :424); best densities in either layout; weight_dev nullable.
 * An emission outside the model, a density outside its mixture, a non-finite feature or weight: AMX_ERR_INVALID naming the first
 * such frame, acc_dev untouched.  Waits for the stream. */
int  amx_mllr_accumulate_dev(amx_mllr* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets, const int* seg_key,
                             const int32_t* emission_dev, const uint32_t* best_density_dev, int best_density_ld, const double* weight_dev,
                             double* acc_dev);
/* FullAdaptor::adaptMixtureSet / ShiftAdaptor::adaptMixtureSet(mixtureSet) (:59-79, :146-170) for one key: out_dev [n_means x D] f32.
 * matrices (host, f64) [n_matrices x D x (D + 1)] (shift: [n_matrices x D]) with their ids, matrix_of_mixture [n_mixtures] as
 * amx_mllr_estimate gives them.  full: per (mean, row) the f64 dot product over [1, m] in ascending column order, fused under
 * AMX_CONTRACT_FMA, narrowed once; shift: f32(shift_d + f64(m_d)).  A mean no mixture reaches is copied.  A matrix id that is not
 * among matrix_ids (the reference's ensure, :64 / :154): AMX_ERR_INVALID.  The caller builds the adapted scorer with amx_gmm_create. */
int  amx_mllr_adapt_means_dev(amx_mllr* h, int n_matrices, const int* matrix_ids, const double* matrices, const int* matrix_of_mixture,
                              float* out_dev);

/* ---- host side (mllr_host.cpp): `acc` is ONE key's part of the flat buffer, amx_mllr_key_size(shape) doubles, host memory. */
/* The reference's binary accumulator behind Core::IoRef's type-name tag, little endian (AdaptorEstimator::write :247-250, then
 * :829-841 / :533-545; AccumulatorBase::write :279-287):
 *   string tag | string clusterId | u32 dimension | Vector<f64> count_ | f64 min-observation | f64 min-silence-observation |
 *   full:  Vector<ZAccumulator> | Vector<GAccumulator> (each Matrix<f64>, f64 count) | map<u16, Matrix<f64>> w_
 *   shift: Vector<f64> count | Vector<Vector<f64>> beta | Vector<Vector<f64>> shift | map<u16, Matrix<f64>> shift_
 * with tag "full-adaptor-viterbi-estimator" / "shift-adaptor-viterbi-estimator".  write gives the file of the accumulating pass:
 * count_ empty (node_count NULL) or the n_ids counts of an estimate, the map as init() leaves it -- every id of map_ids (the tree's
 * ids, ascending) with a 0 x 0 matrix (full) or a 1 x D zero row (shift).  read checks tag, dimension and leaf count against the
 * shape, skips count_ and the map, and returns the two thresholds (nullable); a wrong tag, dimension or leaf count or a truncated
 * file: AMX_ERR_INVALID. */
int  amx_mllr_accumulator_write(const amx_mllr_shape* shape, const double* acc, const char* cluster_id, double min_observation,
                                double min_silence_observation, int n_count, const double* node_count, int n_map_ids, const int* map_ids,
                                const char* path);
int  amx_mllr_accumulator_read(const amx_mllr_shape* shape, const char* path, double* acc, double* min_observation,
                               double* min_silence_observation);
enum { AMX_MLLR_ROOT_FALLBACK = 1, AMX_MLLR_SILENCE_FALLBACK = 2 };
/* adaptor() (:741-827 / :444-531) for one key: propagate in the reference's recursion order (node = left, then += right; :228-248),
 * count > min_observation (strict), per kept node W = Z * pinv(G) (Matrix * Matrix's loop; shift: shift / beta per component), every
 * leaf of the leaf list walked up `previous` to the first node with enough observations, the root-only fallback to
 * adaptationUnitMatrix / the zero shift, the silence mixtures from the LEAF accumulators against min_silence_observation, numbered
 * from n_ids upward, and matrix_of_mixture [n_mixtures] = matrixId[leaf_of_mixture[mixture]].  pinv is Lapack::pseudoInvert's
 * (Math/Lapack/Svd.cc:21-99, dgelsd with rcond 1e-12) by a cyclic Jacobi eigen-decomposition of the symmetrised G with the same
 * truncation (|lambda| <= rcond * max |lambda| dropped); DESIGN.md section 4.19 has the measured distance.  rcond <= 0 takes 1e-12.
 * Out: *n_matrices, matrix_ids ascending (as the std::map iterates) and matrices, room for n_leaf_list + n_silence + 1 of them;
 * node_count [n_ids] (nullable); *flags (nullable).  A tree whose arrays do not describe a tree, a leaf number outside [0, n_leafs),
 * a silence mixture outside the model: AMX_ERR_INVALID. */
int  amx_mllr_estimate(const amx_mllr_shape* shape, const double* acc, const amx_mllr_tree* tree, int n_mixtures, const int* leaf_of_mixture,
                       double min_observation, double min_silence_observation, double rcond, int* n_matrices, int* matrix_ids,
                       double* matrices, int* matrix_of_mixture, double* node_count, int* flags);
/* The adaptor file (FullAdaptor::write / ShiftAdaptor::write :172-177 / :121-126 behind the tag "full-adaptor" / "shift-adaptor"):
 *   string tag | string clusterId | map<u16, Matrix<f64>> | Vector<u16> adaptationMatrixIndex
 * read: capacity max_matrices; *n_matrices, ids, matrices, matrix_of_mixture [n_mixtures] out. */
int  amx_mllr_adaptor_write(const amx_mllr_shape* shape, const char* cluster_id, int n_matrices, const int* matrix_ids, const double* matrices,
                            int n_mixtures, const int* matrix_of_mixture, const char* path);
int  amx_mllr_adaptor_read(const amx_mllr_shape* shape, const char* path, int max_matrices, int* n_matrices, int* matrix_ids, double* matrices,
                           int n_mixtures, int* matrix_of_mixture);

/* ------------------------------------------------------------------ EBW: discriminative training statistics from lattices */

/* The corpus pass of Speech::SegmentwiseGmmTrainer feeding Mm::EbwDiscriminativeMixtureSetEstimator: the arc weights that Fsa::posteriorE
 * left on a lattice become numerator and denominator statistics.  The lattice computation, the arc walk and the per-arc alignments stay
 * with the adapter, which hands over, per segment, its arcs in the order of the reference's depth-first walk, each with one signed f32
 * weight and its alignment as items (frame relative to the segment, emission index).
 *   sides       an arc is numerator if w > weight_threshold, denominator with weight -w if -w > weight_threshold (f32, strict;
 *               Lattice/Accumulator.tcc:66-87 under Speech/SegmentwiseGmmTrainer.cc:160-168), otherwise neither;
 *   collection  per (side, frame, mixture) the f64 sum of the widened arc weights in arc order, then item order
 *               (CachedAcousticAccumulator::process, Collector::collect, Accumulator.tcc:101-107): the order is the input's, so the
 *               collected weights are the reference's in every bit;
 *   density     the best density of the key's mixture for that frame, amx_gmm_best_density_dev's bits (viterbi = 0,
 *               getDensityPosteriorProbabilities, is AMX_ERR_UNSUPPORTED naming `viterbi`); a key without a density is left out;
 *   sums        finish() (:109-115) -> Mm::DiscriminativeMixtureSetEstimator::accumulate / accumulateDenominator
 *               (Mm/DiscriminativeMixtureSetEstimator.cc:187-203): a numerator key adds w to its slot's mixture weight and to its mean's and
 *               covariance's weights, w * x and (w * x) * x to their sums (Mm/MixtureEstimator.cc:92-97); a denominator key adds the
 *               same to the denominator accumulators and w to denWeights_, and NOTHING to the slot's mixture weight:
 *               EbwDiscriminativeMixtureEstimator::accumulateDenominator (Mm/EbwDiscriminativeMixtureEstimator.cc:109-116) overrides the
 *               base class's (Mm/DiscriminativeMixtureEstimator.cc:59-66, `weights_ -= weight`) without calling it, so weights_ of the
 *               EBW estimator is the numerator's weight (its XML writer calls it numerator-weight); tests/golden/make_ebw_golden.py
 *               compiles both functions and the fixture pins this.  x + w * y and x + w * y * y (Mm/Utilities.hh:108-153) are one fused
 *               multiply-add each under amx_set_contract(AMX_CONTRACT_FMA), two roundings otherwise.  The contract of the sums is the
 *               context's at the time of the call; the densities follow the contract the gmm handle took at ITS creation.
 * Order: the reference's finish() walks an unordered_map, which its text does not define.  Here every cell's chain takes its keys in
 * ascending (frame, mixture), per side.  A chain starts from what the buffer holds, so the order continues across calls: a segment gives the same bits
 * alone and in any batch, and a corpus cut into calls between segments gives the bits of one call.  No floating-point atomics.
 * The accumulator is ONE flat f64 buffer the caller owns and zeroes, amx_ebw_accumulator_size() doubles, for one all-reduce:
 *   [ numerator: amx_gmm_accumulate_dev's layout (mixture weights_ | mean weights | mean sums | covariance weights | covariance sums) ]
 *   [ denominator: slot weights (denWeights_) | mean weights | mean sums | covariance weights | covariance sums ] [ objective ]
 * Checked on the device before anything is written, AMX_ERR_INVALID naming the first offender, acc_dev untouched: an item's frame outside
 * its segment, an emission outside the model, an arc weight that is not finite (arcs without items and arcs of neither side included), a
 * feature row that is not finite and that an item of an arc with a side touches.  At most 2^27 frames, arcs and items per call. */
typedef struct amx_ebw amx_ebw;
typedef struct {
    float weight_threshold; /* weight-threshold, default Core::Type<f32>::epsilon */
    int   viterbi;          /* viterbi, default 1; 0 is AMX_ERR_UNSUPPORTED */
} amx_ebw_cfg;
typedef struct {
    long num_mixture_weights, num_mean_weights, num_mean_sums, num_cov_weights, num_cov_sums; /* offsets in doubles */
    long den_density_weights, den_mean_weights, den_mean_sums, den_cov_weights, den_cov_sums;
    long objective, size;
    long n_slots /* sum of the mixtures' densities */, n_means, n_covariances, dim;
} amx_ebw_offsets;
void amx_ebw_cfg_default(amx_ebw_cfg* cfg);
/* the gmm handle must outlive this one; created without a context it gives a host-only handle (sizes and layout).  A scorer that keeps
 * no diagonal-maximum tables on the device (amx_gmm_best_density_dev's condition) is refused here with AMX_ERR_UNSUPPORTED */
int  amx_ebw_create(amx_gmm* gmm, const amx_ebw_cfg* cfg /* NULL: defaults */, amx_ebw** out);
void amx_ebw_destroy(amx_ebw* h);
long amx_ebw_accumulator_size(const amx_ebw* h); /* doubles; 0 for NULL */
int  amx_ebw_layout(const amx_ebw* h, amx_ebw_offsets* out);
/* feats_dev [rows x feats_ld] as the front end left it; segment s owns the rows [frame_offsets[s], frame_offsets[s + 1]) and the arcs
 * [arc_offsets[s], arc_offsets[s + 1]), arc a the items [item_offsets[a], item_offsets[a + 1]); arc_offsets[0] = item_offsets[0] = 0.
 * The tables are host memory.  Synchronises the stream. */
int  amx_ebw_accumulate_dev(amx_ebw* h, const float* feats_dev, int feats_ld, int n_seg, const long* frame_offsets /*[n_seg+1]*/,
                            const long* arc_offsets /*[n_seg+1]*/, const float* arc_weight, const long* item_offsets /*[n_arcs+1]*/,
                            const int32_t* item_frame, const int32_t* item_emission, double* acc_dev);
/* accumulateObjectiveFunction(f32) (Speech/SegmentwiseGmmTrainer.cc:113-116): the widened objective of one segment into the last cell */
int  amx_ebw_accumulate_objective(amx_ebw* h, float objective, double* acc_dev);
/* DIAGNOSTIC, for tests, probes and the statistics channel (not part of the reference's interface; it copies from the handle's workspace):
 * the keys of the last amx_ebw_accumulate_dev in ascending (frame, mixture, side): frame relative to frame_offsets[0], side 0 numerator /
 * 1 denominator, the collected weight and the slot (offset of the best density in the mixture-weight block, -1: no density).  Every array
 * nullable; all NULL: *n_keys only. */
int  amx_ebw_last_keys(const amx_ebw* h, int capacity, int* n_keys, long* frame, int32_t* mixture, int32_t* side, double* weight, int32_t* slot);
/* DIAGNOSTIC, for tests and probes.  amx_ebw_kernel_shape: elements per workgroup of the sort and the scan, keys a chain stages at a time,
 * threads per workgroup (any pointer nullable).  amx_ebw_last_shape: what the last amx_ebw_accumulate_dev ran -- passes and workgroups of
 * the item sort and of the list sort, and whether the scan of a sort's digit table (256 x workgroups) took more than one level; all 0
 * for a call that was refused or ended before the sort */
typedef struct {
    int item_sort_passes, list_sort_passes;
    int item_blocks, list_blocks;
    int item_table_recursed, list_table_recursed;
} amx_ebw_call_shape;
void amx_ebw_kernel_shape(int* block_items, int* stage_keys, int* threads);
int  amx_ebw_last_shape(const amx_ebw* h, amx_ebw_call_shape* out);

/* ---- host side (ebw_host.cpp): `acc` is the flat buffer in host memory, `topology` the model the statistics were accumulated with
 * (its means, variances and weights are not read).  amx_ebw_topology_accumulator_size: amx_ebw_accumulator_size from the topology alone
 * (0 for a topology that is refused).
 * The file is the reference's binary estimator file of Mm::EbwDiscriminativeMixtureSetEstimator: the "MIXSET" layout under the magic "DTACC"
 * (Mm/DiscriminativeMixtureSetEstimator.hh:42-44; eight bytes, the three behind the letters zero), version 2
 * (Mm/AbstractMixtureSetEstimator.cc:404-508), every mean and covariance record followed by its denominator accumulator
 * (Mm/EbwDiscriminativeGaussDensityEstimator.cc:55-58, :150-153), every mixture record by its denWeights_
 * (Mm/EbwDiscriminativeMixtureEstimator.cc:148-154), and the objective function as the last f64
 * (Mm/DiscriminativeMixtureSetEstimator.cc:115-119): the file RASR's accumulate, combine-mixture-set-estimators and estimate actions exchange.
 * Its bytes are those the reference's write chain makes, compiled by tests/golden/make_ebw_golden.py (ref_ebw.npz); the reference's
 * reader has not been run on a file from here.  read requires the file's topology to equal the
 * model's, its version to be 2 and the file to end behind the objective; a file that is refused leaves `acc` untouched.
 * combine is the file-level sum of AbstractMixtureSetEstimator::accumulate(is, os) (:170-300) for two estimators: acc += add in every
 * cell, the objective included (DiscriminativeMixtureSetEstimator.cc:162-177); an entry that is not finite is AMX_ERR_INVALID and
 * nothing is added. */
long amx_ebw_topology_accumulator_size(const amx_gmm_model* topology);

/* The EBW update: Mm::DiscriminativeMixtureSetEstimator::estimate (Mm/DiscriminativeMixtureSetEstimator.cc:136-160) for
 * Mm::EbwDiscriminativeMixtureSetEstimator and, with an i-smoothing set, ...WithISmoothing, operation by operation in f64:
 *   previous set   distributed by index (:51-86); here its topology must EQUAL `topology` (the reference compares the counts only);
 *   removal        removeDensitiesWithLowWeight's discriminative rule (Mm/DiscriminativeMixtureEstimator.cc:34-49): weights_ -- the
 *                  numerator's weight, see above -- against min_observation_weight, the previous mixture weight against
 *                  min_relative_weight, the heaviest density kept, `--densityMax` after EVERY removal as the reference has it; the
 *                  survivors renumbered in order of first appearance, as amx_gmm_estimate renumbers;
 *   constants      Mm/IterationConstants.cc: Xi and beta, sigma-minimum (or sigma_minimum_factor times the smallest previous variance),
 *                  minimumDk, global-rwth / local-rwth, step-size, minimum-icd, the scaling by the previous mixture weight;
 *   means, covariances   Mm/EbwDiscriminativeGaussDensityEstimator.cc:73-99, :165-207: the narrowing to f32, applyMinimumVariance, the
 *                  previous mean where dtWeight + D <= 0;
 *   weights        the Cambridge scheme of estimateMixtureWeights (Mm/EbwDiscriminativeMixtureEstimator.cc:39-91): number_of_iterations,
 *                  the clamp to 0, the normalisation and its vanishing-sum fallback; then Mixture::normalizeWeights;
 *   i-smoothing    with `ismoothing` given: i_smoothing_means / i_smoothing_weights enter dtSum, dtWeight, iSum and weight(dns)
 *                  (:114-121, :222-229, Mm/ISmoothingGaussDensityEstimator.cc:56-71, Mm/EbwDiscriminativeMixtureEstimator.hh:83-85), and
 *                  info->i_smoothing_objective is ISmoothing*::getObjectiveFunction on the NEW set (Mm/ISmoothingMixtureSetEstimator.cc:96-115);
 *   finalize       with min_relative_weight != 0, Mixture::removeDensitiesWithLowWeight on the new set (Mm/Mixture.cc:109-129; its
 *                  densityIndexWithMaxWeight compares two iterators, so no density is protected there).
 * cfg->contract says which build of the reference is followed (AMX_CONTRACT_OFF | AMX_CONTRACT_FMA: the sums the -march=native build
 * fuses, read off tests/golden/ref_ebw.npz).  Sums that the reference takes in the order of a hash table -- the densities of a shared
 * covariance in minimumDk, the means of a covariance in the covariance estimate and iSum -- are taken in ascending (new) index here;
 * DESIGN.md section 6 has the measured distance.  The result is a mixture set like amx_gmm_estimate's.
 * Refused, amx_last_error naming the cause: AMX_ERR_UNSUPPORTED for iteration constants of type cambridge (maximumRoot starts with
 * require(false)), local-rwth on a model where a mixture's densities use more than one covariance (the result would depend on the hash
 * walk), a density shared by two mixtures (the reference requires this) or a mean shared by two densities (the iteration constant of the
 * mean would be the hash walk's last), the Rprop estimator, viterbi = 0; AMX_ERR_INVALID for a non-finite accumulator, a topology that
 * differs, a summed weight <= 0 or an estimated variance <= 0 (the reference's verify), an iteration constant that is not finite. */
enum { AMX_EBW_IC_GLOBAL_RWTH = 0, AMX_EBW_IC_LOCAL_RWTH = 1, AMX_EBW_IC_CAMBRIDGE = 2 };
enum { AMX_EBW_ESTIMATOR_EBW = 0, AMX_EBW_ESTIMATOR_RPROP = 1 };
typedef struct {
    double min_observation_weight;    /* minimum-observation-weight, 5 */
    double min_relative_weight;       /* minimum-relative-weight, 0 */
    double min_variance;              /* minimum-variance, 0 (compared and stored as f32) */
    int    normalize_mixture_weights; /* normalize-mixture-weights, 1 */
    int    iteration_constants;       /* iteration-constants.type, global-rwth */
    double step_size;                 /* step-size, 1.1 */
    double minimum_icd;               /* minimum-icd, 1 */
    double beta;                      /* icb.xi.beta, 1 */
    double sigma_minimum;             /* icb.sigma-minimum; negative (the default here): sigma_minimum_factor * smallest previous variance */
    double sigma_minimum_factor;      /* icb.sigma-minimum-factor, 1e-5 */
    int    number_of_iterations;      /* mixture-estimator.number-of-iterations, 100 */
    double i_smoothing_means;         /* i-smoothing-means, 0 */
    double i_smoothing_weights;       /* i-smoothing-weights, 0 */
    int    viterbi;                   /* 1 */
    int    estimator;                 /* AMX_EBW_ESTIMATOR_EBW */
    int    contract;                  /* AMX_CONTRACT_OFF */
} amx_ebw_estimate_cfg;
typedef struct {
    double i_smoothing_objective; /* 0 without an i-smoothing set */
    double sigma_minimum;
    int    n_removed, n_clamped /* (mixture, density) pairs whose weight an iteration set to 0 */, n_mean_fallback, n_floored;
} amx_ebw_estimate_info;
void amx_ebw_estimate_cfg_default(amx_ebw_estimate_cfg* cfg);
/* previous / ismoothing: views of mixture sets on the topology (amx_mixture_set_view gives one); ismoothing, info and
 * iteration_constants ([topology->n_mean] doubles, filled by NEW mean index) are nullable */
int  amx_ebw_estimate(const amx_gmm_model* topology, const double* acc, const amx_gmm_model* previous, const amx_gmm_model* ismoothing,
                      const amx_ebw_estimate_cfg* cfg /* NULL: defaults */, amx_mixture_set** out, amx_ebw_estimate_info* info,
                      double* iteration_constants);
int  amx_ebw_accumulator_write(const amx_gmm_model* topology, const double* acc, const char* path);
int  amx_ebw_accumulator_read(const amx_gmm_model* topology, const char* path, double* acc);
int  amx_ebw_accumulator_combine(const amx_gmm_model* topology, double* acc, const double* add);

/* ------------------------------------------------------------------ Lattice arc posteriors */

/* The forward-backward pass over word lattices that the discriminative trainers start from, for a batch of lattices per call, the
 * results left on the device: Fsa::posterior64 (Fsa/Sssp.cc:95-225; the MMI GMM trainer, Nn::MmiSegmentwiseNnTrainer,
 * Nn/MmiSegmentwiseNnTrainer.cc:36-60, Lattice::posterior) and Fsa::posteriorE (Sssp.cc:231-375; the MPE GMM trainer,
 * Speech/SegmentwiseGmmTrainer.cc:138-169, Nn::MeSegmentwiseNnTrainer), in f64 in the log semiring.
 *   potentials   StatePotentials64DfsState::finishState (Sssp.cc:95-138): a state's potential is a function of its outgoing arcs IN ARC
 *                ORDER, of the targets' potentials and of its final weight.  Start value: the final weight widened from f32, or
 *                Zero = Core::Type<f64>::max (:67).  score = potential[target] + f32(weight), an infinite score becomes f64 max; the
 *                search uses `<=`, so the LAST minimal arc is left out of the sum; the sum starts with exp(min - final) only for a final
 *                state whose minimum an arc took; the other arcs add exp(min - score) in arc order; min - log1p(sum), clamped to Zero.
 *   forward      the same function on transpose(fsa) (Fsa/tRational.cc:594-689): a state's transposed arcs stand in the order in which
 *                TransposeDfsState::discoverState appended them, that is the DISCOVER order of their source states in the stack walk of
 *                Fsa/tDfs.cc:21-68 (every white target is pushed, a state is discovered when it is popped) and, within a source, the
 *                source's arc order; a new initial state has one arc per final state in discover order, weighted with the final weight;
 *                the old initial state is final with weight one.
 *   arcs         f32(min(fw[s] + f32(w) + bw[target] + totalInv, f32 max)) (:156-159); a final state f32(min(fw[s] + final + totalInv,
 *                f32 max)), or 0 without arcs (:160-165); totalInv = -bw[initial], or 0 with normalize = 0 (:185).
 *   AMX_LATPOST_PROB         then Fsa::expm (Fsa/Arithmetic.cc:47-61): isinf(w) ? 0 : f32(exp(-(f64)w)) -- the f64 overload, as the
 *                reference's translation unit resolves it (tests/golden/make_latpost_golden.py compiles the text and records it).
 *   AMX_LATPOST_EXPECTATION  StatePotentialsEDfsState::finishState (:254-288): strict minimum, denSum takes EVERY arc (log1p(denSum - 1)),
 *                numSum += p * (risk + generalized[target]) -- a contraction site of the reference's default build: one fused multiply-add
 *                under amx_set_contract(AMX_CONTRACT_FMA), two roundings otherwise (the context's setting at the time of the call) --,
 *                written only if denSum > 0, generalized clamped to +-Zero.  An arc: f32(exp(-(f64)logPosterior) * risk) with
 *                risk = f32(min(gfw[s] + f32(r) + gbw[target] - normalization, f32 max)) (:305-314, :352-362), normalization =
 *                gbw[initial] with v_normalized, else 0; a final state f32(exp(-finalLogPosterior) * f32(min(final_risk - normalization,
 *                f32 max))), the risk factor 0 without arcs.  totalInv is -bw[initial] whatever `normalize` says (:340).
 * Input: CSR tables in host memory.  Segment g owns the states [state_offsets[g], state_offsets[g + 1]), state ids are dense per segment
 * (arc_target and initial are ids within the segment), state i (counted over the call) owns the arcs [arc_offsets[i], arc_offsets[i + 1])
 * in the automaton's own order.  Outputs: f32 on the device, arc_out_dev[n_arcs] in the input's arc order, final_out_dev[n_states].
 * Where the reference defines nothing, the library chooses:
 *   - a state the walk from the initial state does not reach has backward potential Zero, and a state the transposed walk does not reach
 *     (the reference's forwardPotentials_ vector may not even have grown that far) has forward potential Zero; the arcs that leave such
 *     a state are counted in info.undefined_arcs, the states in info.undefined_states; their outputs follow from Zero by the formulas;
 *   - a state that is not final has final_out f32 max (LOG) or 0 (PROB, EXPECTATION);
 *   - a segment in which no final state is reached (the reference's transpose returns an empty automaton) has reason
 *     AMX_LATPOST_NO_FINAL and every output dead: f32 max (LOG) or 0; it is not an error.
 * Order: every sum is one chain in the order above and depends on the segment alone: a segment gives the same bits alone and in any
 * batch.  No floating-point atomics, no tree sums.  exp and log1p are the device library's (1 ulp class), so values are close to, not
 * equal to, the host's; the bars are measured from the reference's arithmetic (tests/golden/ref_latpost.npz).
 * Refused with AMX_ERR_INVALID naming the first offender, outputs untouched: a cycle anywhere in a segment (the reference requires
 * PropertyAcyclic), a target outside its segment, an initial state out of range, a NaN weight or risk, EXPECTATION without risks,
 * offsets that do not ascend.  +-inf weights follow the reference (isinf(score) -> f64 max). */
enum { AMX_LATPOST_LOG = 0, AMX_LATPOST_PROB = 1, AMX_LATPOST_EXPECTATION = 2 };
enum { AMX_LATPOST_OK = 0, AMX_LATPOST_NO_FINAL = 1 };
enum { AMX_LATPOST_POTENTIALS_AUTO = 0, AMX_LATPOST_POTENTIALS_GLOBAL = 1 };
typedef struct amx_latpost amx_latpost;
typedef struct {
    int mode;         /* AMX_LATPOST_LOG */
    int normalize;    /* 1; read by LOG and PROB */
    int v_normalized; /* 1; read by EXPECTATION */
    int tolerance;    /* 100: posterior-tolerance of the flow comparison */
    int potentials;   /* AMX_LATPOST_POTENTIALS_AUTO: in LDS while a segment's states fit (amx_latpost_kernel_shape); _GLOBAL: always in
                         global memory (tests: both paths give the same bits) */
} amx_latpost_cfg;
typedef struct {
    double total_inv;     /* -bw[initial] (Posterior64Automaton::totalInv) */
    float  total_inv_f32; /* LOG, PROB: clamped from below at f32 min (:206); EXPECTATION: narrowed (:328-330) */
    float  expectation;   /* EXPECTATION: f32(gbw[initial]); 0 otherwise */
    float  forward_flow, backward_flow;
    int    flows_agree;    /* Core::isAlmostEqual(fwd, bwd, tolerance) (:188), EXPECTATION: isAlmostEqualUlp (:343) */
    int    vanishing_flow; /* isAlmostEqualUlp(total_inv_f32, f32 min, tolerance) (Nn/MmiSegmentwiseNnTrainer.cc:41) */
    int    reason;         /* AMX_LATPOST_OK | AMX_LATPOST_NO_FINAL */
    int    states_reached, arcs_reached;      /* by the walk from the initial state */
    int    states_coreached;                  /* by the transposed walk (the new initial state not counted) */
    int    undefined_states, undefined_arcs;  /* states the transposed walk does not reach, and the arcs that leave them */
    int    levels_forward, levels_backward;   /* barriers of the two workgroups */
} amx_latpost_info;
void amx_latpost_cfg_default(amx_latpost_cfg* cfg);
/* ctx NULL: a host-only handle (amx_latpost_plan_host) */
int  amx_latpost_create(amx_ctx* ctx, const amx_latpost_cfg* cfg /* NULL: defaults */, amx_latpost** out);
void amx_latpost_destroy(amx_latpost* h);
/* the potentials kernel's launch shape (tests pick their sizes around it): threads of a workgroup, the largest number of states of a
 * segment (the forward walk's new initial state included: n + 1 <= lds_states) whose potentials live in LDS, and the number of arcs from
 * which a state is shared by a wave instead of taken by one lane */
void amx_latpost_kernel_shape(int* threads, int* lds_states, int* wave_arcs);
/* arc_risk / final_risk: EXPECTATION only, else ignored (NULL allowed); final_weight / final_risk are read where final_flag is set.
 * info [n_seg] in host memory, nullable.  Synchronises the stream. */
int  amx_latpost_run_dev(amx_latpost* h, int n_seg, const long* state_offsets /*[n_seg+1]*/, const long* arc_offsets /*[n_states+1]*/,
                         const int32_t* arc_target, const float* arc_weight, const float* arc_risk, const int32_t* initial /*[n_seg]*/,
                         const uint8_t* final_flag, const float* final_weight, const float* final_risk, float* arc_out_dev,
                         float* final_out_dev, amx_latpost_info* info);
/* The host plan alone (no device): the checks above and, per state counted over the call, discover_index (position in the reference's
 * discover order, -1: not reached), level_backward / level_forward (the level at which the state's potential is computed, -1: not walked),
 * in_offsets [n_states + 1] / in_arc: the transposed state's arcs as indices of input arcs, in the reference's order; final_order: per
 * segment, from state_offsets[g] on, the reached final states in discover order (the new initial state's arcs), then -1.  level_super
 * [n_seg]: the new initial state's level (-1 with AMX_LATPOST_NO_FINAL).  Every output nullable; info's discrete fields are filled. */
int  amx_latpost_plan_host(const amx_latpost* h, int n_seg, const long* state_offsets, const long* arc_offsets, const int32_t* arc_target,
                           const float* arc_weight, const float* arc_risk, const int32_t* initial, const uint8_t* final_flag,
                           const float* final_weight, const float* final_risk, int32_t* discover_index, int32_t* level_backward,
                           int32_t* level_forward, int32_t* level_super, long* in_offsets, int32_t* in_arc, int32_t* final_order,
                           amx_latpost_info* info);
/* DIAGNOSTIC (tests, probes): the potentials of the last amx_latpost_run_dev, per state counted over the call; generalized_*: EXPECTATION
 * (else zeros).  Every array nullable. */
int  amx_latpost_last_potentials(const amx_latpost* h, long n_states, double* forward, double* backward, double* generalized_forward,
                                 double* generalized_backward);
/* DIAGNOSTIC (tools/latpost_probe.py): host wall time of the last amx_latpost_run_dev's plan and of packing and uploading its tables, in ms;
 * the kernels' times are the event timers' (amx_profile_get "latpost_potentials", "latpost_arcs") */
int  amx_latpost_last_timing(const amx_latpost* h, double* plan_ms, double* upload_ms);

/* ------------------------------------------------------------------ NN sequence-discriminative training (MMI, ME)
 * Nn::SegmentwiseNnTrainer in full-batch mode (Nn/SegmentwiseNnTrainer.cc:121-250 processWordLattice) for a batch of segments per
 * call, on an amx_nntrain handle whose mask has BASE (and GRADIENT for anything but the base statistics): the handle's weights, its
 * workspace and its accumulator layout are shared, so amx_nnstat_write / _combine and amx_nntrain_estimate take the result as it is.
 * The model comes with the log prior already removed from the top bias (Nn/SharedNeuralNetwork.cc:40-90).  What stays with the
 * adapter: numerator extraction and Lattice::best (emission_dev is their result), the language-model part of the arc scores and the
 * scales, the lattice forward-backward (amx_latpost_run_dev on the combined scores), `skip`, and objective[s].
 *
 * 1. amx_nnseq_forward_dev: the forward pass of amx_nntrain_accumulate_dev for every segment; feats_dev rows are absolute
 *    ([frame_offsets[s], frame_offsets[s + 1]) belongs to segment s).  In the workspace segment s starts at a row that is a multiple
 *    of AMX_NNTRAIN_CHUNK; the rows between two segments are zero in every layer input.  The sum of the padded lengths is at most
 *    AMX_NNTRAIN_MAX_FRAMES.  Every layer's input and the linear top output are kept until the next forward.
 * 2. amx_nnseq_arc_scores_dev: EmissionLatticeRescorerAutomaton::_score (Nn/EmissionLatticeRescorer.cc:208-231): per arc one f32 chain
 *    from 0, score -= out[class_to_output[e], t] in item order; an arc without items keeps 0.  Tables as amx_ebw_accumulate_dev's, in
 *    host memory (item_frame relative to the segment); the scores stay on the device.  Needs the linear top output (before an
 *    accumulate with smoothing has replaced it by the softmax).
 * 3. amx_nnseq_accumulate_dev: the rest of processWordLattice.  A pass is one accumulateStatisticsOnLattice (:619-627) over its own
 *    arc and item tables with arc_weight_dev as amx_latpost_run_dev left it:
 *      collection  an arc counts if (f64)w > weight_threshold, w = the f32 arc weight, times (f32)-1 first with `negate`
 *                  (Fsa::multiply; Lattice/Accumulator.tcc:66-87); per (frame, emission) the widened weights are summed in f64 in arc
 *                  order, then item order (Nn/LatticeAccumulators.hh:82-93); E[o, t] = (f32)((f64)E[o, t] + factor * collected),
 *                  o = class_to_output[e] (LatticeAccumulators.cc:45-49), one write per cell and pass, passes in the order given: the
 *                  reference's bits whatever its unordered_map walk was.  A stable key sort, no floating-point atomics.
 *      roles       AMX_NNSEQ_ADD; AMX_NNSEQ_ADD_REJECT: then w[t] = 0 where E[alignment[t], t] < frame_rejection_threshold (f32;
 *                  Nn/MmiSegmentwiseNnTrainer.cc:78-86), counted per segment; a cell that is not >= 0 (verify_ge) refuses the call;
 *                  AMX_NNSEQ_ADD_REJECT_CLEAR: then E = 0 (Nn/MeSegmentwiseNnTrainer.cc:69-100).
 *                  MMI: den PROB +1 [reject], num PROB -1.  ME: EXPECTATION -1, the same tables negated +1.  ME with rejection: the
 *                  MMI denominator +1 [reject, clear] in front.
 *      alignment   alignment[t] = class_to_output[emission_dev[t]] (AlignmentAccumulator); emission_dev is indexed by frame -
 *                  frame_offsets[0]; a frame with 0xffffffff: "alignment vector failed", the segment is skipped and counted.
 *                  w[t] = class_weights[alignment[t]] (:740-745; weights of 1 give the unweighted trainer's bits).
 *      smoothing   if ce_smoothing_weight > 0 (:630-692): top += prior_scale * log_prior where prior_scale > 0 (one fused multiply-add
 *                  per element, the convention stated for the regulariser's axpy), softmax as amx_ffnn_forward_dev(..,
 *                  AMX_NN_TOP_SOFTMAX); E *= (f32)(1.0 - lambda); E = fmaf(lambda, p, E); E[alignment[t], t] += -lambda; the CE objective
 *                  of a segment is one f32 chain obj -= logf(p[alignment[t], t]) * w[t] in frame order.  lambda == 1: the passes are
 *                  not run, E starts from zero (:159-162).
 *      gradient    E's columns times w (multiplyColumnsByScalars), backpropagation without a clip, gradients through the kernels of
 *                  amx_nntrain_accumulate_dev.
 *      base        classification errors of the top output as it then stands (softmax or linear) against the alignment, observations,
 *                  total weight = sum |w|, objective[s] (f32, widened) -- the adapter forms it from amx_latpost_info.total_inv_f32 as
 *                  the two trainers do (MMI: f32(den) - f32(num); ME: -f32(totalInv)).
 * Order: a segment's gradient is formed in f32 from zero over its own chunks, as one amx_nntrain_accumulate_dev call forms it, then
 * widened and added into acc_dev in segment order: a segment gives the same bits alone and in any batch, a batch the bits of one call
 * per segment.  The f64 buffer is the library's choice, as for amx_nntrain_*: the reference's only instantiation
 * (SegmentwiseNnTrainer<f32>) sums across segments in f32 inside BLAS, in no defined order.
 * Checked on the device before acc_dev is written, AMX_ERR_INVALID naming the first offender: an item's frame outside its segment, an
 * emission >= n_classes or of a disregarded class, an arc weight that is not finite, a label out of range or of a disregarded class, a
 * negative cell under the rejection test.  Segments flagged in skip add nothing and are not checked.
 * A segment whose alignment holds 0xffffffff is marked before the labels are checked, so nothing of it is checked either.
 * Keys: the reference's Collector keys on (frame, emission), the library on (frame, class_to_output[emission]).  The two are the same
 * keys because amx_nntrain_create refuses a class_to_output in which two classes share an output ("no one-to-one correspondence").
 * Limits: at most 8 passes per call; at most 2^27 - 1 arcs and 2^27 - 1 items per table.
 * The workspace is the nntrain handle's: forward, scores and accumulate of one batch belong together.  Any amx_nntrain_accumulate_dev /
 * amx_nntrain_step_* call or another amx_nnseq handle's forward on the same nntrain handle in between takes the workspace, and the
 * scores / accumulate call that follows returns AMX_ERR_STATE asking for the forward pass again.
 * AMX_ERR_UNSUPPORTED naming the option: the stochastic per-segment update (full_batch = 0), accumulate_prior (the adapter has it from
 * emission_dev and AMX_NNSTAT_CLASS_COUNTS), allophone-state labels (label_type != 0), and what amx_nntrain_create refuses. */
typedef struct amx_nnseq amx_nnseq;
enum { AMX_NNSEQ_ADD = 0, AMX_NNSEQ_ADD_REJECT = 1, AMX_NNSEQ_ADD_REJECT_CLEAR = 2 };
enum { AMX_NNSEQ_SEG_OK = 0, AMX_NNSEQ_SEG_SKIPPED = 1, AMX_NNSEQ_SEG_NO_ALIGNMENT = 2 };
typedef struct {
    double       weight_threshold;          /* weight-threshold (an Mm::Weight), default Core::Type<f32>::epsilon */
    float        ce_smoothing_weight;       /* 0..1, default 0 */
    float        frame_rejection_threshold; /* 0..1, default 0 = off */
    const float* log_prior;                 /* nullable [n_outputs]; read by the smoothing alone */
    float        prior_scale;               /* default 0 */
    int          full_batch;                /* default 1; 0 is AMX_ERR_UNSUPPORTED */
    int          accumulate_prior;          /* default 0; 1 is AMX_ERR_UNSUPPORTED */
    int          label_type;                /* default 0 = emission indices; anything else is AMX_ERR_UNSUPPORTED */
    int          keep_lattice_error;        /* DIAGNOSTIC: keep a copy of E as the passes left it (amx_nnseq_get_error_signal, layer -1) */
} amx_nnseq_cfg;
typedef struct {
    const long*    arc_offsets;    /* host [n_seg + 1] */
    const long*    item_offsets;   /* host [n_arcs + 1] */
    const int32_t* item_frame;     /* host, relative to the segment */
    const int32_t* item_emission;  /* host */
    const float*   arc_weight_dev; /* device [n_arcs] */
    int            negate;
    double         factor;
    int            role;           /* AMX_NNSEQ_ADD* */
} amx_nnseq_pass;
typedef struct {
    int      segments_processed, segments_skipped, segments_without_alignment;
    long     observations, rejected_observations;
    float    ce_objective;   /* ceObjectiveFunction_: the segments' values added in f32 in segment order */
    int*      seg_reason;       /* nullable [n_seg]: AMX_NNSEQ_SEG_* */
    uint32_t* seg_errors;       /* nullable [n_seg] */
    uint32_t* seg_rejected;     /* nullable [n_seg] */
    float*    seg_ce_objective; /* nullable [n_seg] */
} amx_nnseq_info;
void amx_nnseq_default_cfg(amx_nnseq_cfg* cfg);
/* the nntrain handle must outlive this one; on a host-only nntrain handle this is a host-only handle (the checks alone) */
int  amx_nnseq_create(amx_nntrain* train, const amx_nnseq_cfg* cfg, amx_nnseq** out);
void amx_nnseq_destroy(amx_nnseq* h);
int  amx_nnseq_forward_dev(amx_nnseq* h, const float* feats_dev, int feats_stride, int n_seg, const long* frame_offsets /*[n_seg+1]*/);
int  amx_nnseq_arc_scores_dev(amx_nnseq* h, const long* arc_offsets /*[n_seg+1]*/, const long* item_offsets /*[n_arcs+1]*/,
                              const int32_t* item_frame, const int32_t* item_emission, float* arc_score_dev);
/* skip [n_seg] nullable; objective [n_seg] host f32; info nullable, its arrays nullable.  Synchronises the stream. */
int  amx_nnseq_accumulate_dev(amx_nnseq* h, int n_pass, const amx_nnseq_pass* passes, const uint32_t* emission_dev, const uint8_t* skip,
                              const float* objective, double* acc_dev, amx_nnseq_info* info);
/* DIAGNOSTICS for tests and probes.  workspace_row: the workspace row of a segment's first frame after the last forward.  The getters
 * copy rows [row, row + n) of the workspace: get_top which = 0 the linear top output, 1 the softmax p (AMX_ERR_STATE if the workspace
 * holds the other) [n x n_outputs]; get_error_signal E of a layer [n x out_dim] as the last accumulate left it (the top layer's after
 * smoothing and weighting), layer -1: the copy cfg.keep_lattice_error keeps [n x n_outputs]; get_weights w [n]. */
int  amx_nnseq_workspace_row(const amx_nnseq* h, int segment, int* row);
int  amx_nnseq_get_top(amx_nnseq* h, int which, int row, int n, float* out);
int  amx_nnseq_get_error_signal(amx_nnseq* h, int layer, int row, int n, float* out);
int  amx_nnseq_get_weights(amx_nnseq* h, int row, int n, float* out);
/* elements per workgroup of the collection's sort, arcs a workgroup of the score kernel takes, items a wave of it stages at a time,
 * threads per workgroup (any pointer nullable) */
void amx_nnseq_kernel_shape(int* sort_block_items, int* score_block_arcs, int* score_stage_items, int* threads);
/* passes and workgroups of the sort of the last accumulate's LAST pass; 0 where none ran */
int  amx_nnseq_last_shape(const amx_nnseq* h, int* sort_passes, int* sort_blocks);

#ifdef __cplusplus
}
#endif
#endif
