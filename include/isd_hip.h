/*
 * isd_hip.h -- C ABI of libisd_hip.so: the MI355X (gfx950) hot path of the
 * EEG imagined-speech decoder.
 *
 * The reference (kidusabe1/Imagined-Speech-Decoding) is pure Python and has no
 * FFI; its boundaries for this path are duck-typed Python call sites
 * (SURVEY.md 8b).  Each entry point below names the reference call it
 * replaces.  Conventions (all functions):
 *   - plain pointers + sizes only, no torch types; every data pointer is a
 *     DEVICE pointer owned by the caller unless the name says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - nothing synchronises the host, allocates device memory or launches
 *     threads inside a *_forward / *_backward call (graph-capturable);
 *   - return 0 on success, a negative ISD_ERR_* otherwise; the message of the
 *     last failure on the calling thread is isd_last_error();
 *   - plans are opaque, immutable after create, shareable across streams;
 *   - a launch receives its workspace as a bare pointer.  The matching size query
 *     (*_work_bytes, *_workspace_bytes) answers exactly what the launch addresses
 *     plus the slack its comment names: both read one layout (csrc/common.h,
 *     WorkCarver).  A negative answer is an ISD_ERR_* code.
 */
#ifndef ISD_HIP_H
#define ISD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISD_ABI_VERSION 1

enum {
  ISD_OK = 0,
  ISD_ERR_INVALID = -1,     /* bad argument / shape */
  ISD_ERR_UNSUPPORTED = -2, /* valid request this build cannot run */
  ISD_ERR_HIP = -3,         /* HIP runtime error (message has hipGetErrorString) */
  ISD_ERR_NO_DEVICE = -4    /* no gfx950 device visible */
};

int isd_abi_version(void);
const char* isd_last_error(void);
/* Measurement aid (bench.py): one wave reads the shader-clock counter and the constant-rate counter around a spin of
 * about `spin_us` microseconds and stores {shader ticks, constant-rate ticks} as two uint64 at `out` (device memory);
 * shader MHz = ticks[0] / ticks[1] * isd_wall_clock_khz() / 1000.  Launch it on a second stream beside the kernels
 * being timed. */
int isd_shader_clock_probe(uint64_t* out, int spin_us, void* stream);
int isd_wall_clock_khz(void);
/* The exact, order-independent sum of n fp32 values rounded once to fp64: the accumulator the BatchNorm heads keep
 * their batch sums in (64-bit integer atomics on a fixed-point image of the partials; the same bits on every run --
 * src/fast/utils.py:104-114 asks for deterministic training).  `workspace`: isd_exact_sum_workspace_bytes() bytes. */
int64_t isd_exact_sum_workspace_bytes(void);
int isd_exact_sum(const float* x, int64_t n, double* out, void* workspace, void* stream);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int isd_device_count(void);

/* ------------------------------------------------------------------------
 * Filterbank: IIR band-pass cascade, one Butterworth SOS cascade per band.
 * Replaces (spec S step 1-2) the scipy path
 *   butter(order, band, 'bandpass', fs, output='sos') ; sosfilt(sos, x, axis=-1)
 * anchored on notebooks/svm_baseline.ipynb:238 (the repo's only band-pass).
 * Sections are given in "resonator form": every section is
 *   H(z) = (1 - z^-2) / (1 + a1 z^-1 + a2 z^-2)   and one gain per band,
 * which is what a Butterworth band-pass factors into (zeros at z = +1, -1).
 * ---------------------------------------------------------------------- */
typedef struct isd_fb_plan isd_fb_plan;

enum { ISD_FB_F32 = 0, ISD_FB_F64 = 1, ISD_FB_AUTO = 2, ISD_FB_MIXED = 3 /* reported only */ };

/* a12  : host, [n_bands][n_sections][2] doubles (a1, a2)
 * gain : host, [n_bands] doubles
 * precision: arithmetic of the in-chunk recursion (the cross-chunk state scan
 *            is always fp64); AUTO decides PER BAND: a band whose poles are too
 *            close to z=1 for fp32 to keep 1e-4 runs in fp64, the others in fp32
 *            (see DESIGN.md).  n_sections <= 8. */
int isd_fb_plan_create(isd_fb_plan** out, int n_bands, int n_sections,
                       const double* a12, const double* gain, int precision);
int isd_fb_plan_destroy(isd_fb_plan* plan);
int isd_fb_plan_precision(const isd_fb_plan* plan); /* resolved ISD_FB_F32 / F64 / MIXED */

/* x [B][C][T] f32  ->  y [B][n_bands][C][T] f32   (zero initial state, causal) */
int isd_fb_forward(const isd_fb_plan* plan, const float* x, float* y,
                   int64_t B, int64_t C, int64_t T, void* stream);

/* ------------------------------------------------------------------------
 * STFT with the scipy-legacy defaults used at
 *   scripts/global_shap_analysis.py:132  scipy.signal.stft(sig, fs, nperseg=64, noverlap=32)
 * (periodic Hann, zero extension by nperseg/2, zero padding to whole frames,
 * one-sided rfft, scaling='spectrum'), and the inclusive band aggregation of
 *   scripts/global_shap_analysis.py:151-156.
 * nperseg must be a power of two in [8, 4096]; 0 <= noverlap < nperseg.
 * ---------------------------------------------------------------------- */
typedef struct isd_stft_plan isd_stft_plan;

int isd_stft_plan_create(isd_stft_plan** out, int T, int nperseg, int noverlap);
int isd_stft_plan_destroy(isd_stft_plan* plan);
int isd_stft_plan_frames(const isd_stft_plan* plan); /* J */
int isd_stft_plan_bins(const isd_stft_plan* plan);   /* nperseg/2 + 1 */

/* x [R][T] f32 -> Z [R][bins][J] complex64 (interleaved re,im), scipy layout */
int isd_stft_forward(const isd_stft_plan* plan, const float* x, float* Z,
                     int64_t R, void* stream);

enum {
  ISD_BP_MAGNITUDE = 0, /* mean |Z|        (global_shap_analysis.py:135,156) */
  ISD_BP_POWER = 1,     /* mean |Z|^2                                        */
  ISD_BP_LOGPOWER = 2   /* log(mean |Z|^2 + eps)   (spec S steps 4-5)        */
};

/* Band aggregation of per-band filtered signals.
 * y [B][n_bands][C][T] f32 -> feat [B][n_bands][C][J] f32; band b of the
 * input is reduced over its own bins klo[b]..khi[b] (inclusive, host int
 * arrays; khi < klo = empty band -> 0 before the log).
 * With n_bands_in == 1 the same signal y [B][1][C][T] is reduced over every
 * band (the reference's use: one trace, five bands) -> feat [B][n_bands][C][J]. */
int isd_stft_bandpower(const isd_stft_plan* plan, const float* y, float* feat,
                       int64_t B, int64_t C, int n_bands_in, int n_bands,
                       const int* klo, const int* khi, int mode, float eps, void* stream);
/* The kernel that the calling thread's last isd_stft_bandpower launched, as family + 16 * instance:
 *   0 none yet;
 *   1 / 17 the direct DFT (nperseg 64, hop 32, T <= 512, per-band input): bandpower_direct_kernel<MAG, FULL> with
 *   FULL = false / true (MAG follows the mode);
 *   2 + 16 KB = 66 / 82 / 98 / 130 the block sums (hop 32 or 64 = the plan's, nperseg = 2^a hop with 4..64 blocks per
 *   frame, T <= 64 hop, every band 1..6 interior bins, per-band input): bandpower_blocksum_kernel<hop, KB>, KB = 4 / 5 /
 *   6 / 8 slots for the widest band's 2 / 3 / 4 / 5..6 bins and their two Hann neighbours;
 *   3 the radix-2 FFT with the band reduction (everything else, n_bands_in == 1 included).
 * A call that fails its argument checks or has B == 0 leaves the value.  For tests: a fall-back to another kernel must
 * not pass for the intended one. */
int isd_stft_bandpower_last_path(void);

/* Fused spec-S feature extractor: filterbank -> STFT -> log band power without
 * materialising the filtered signals.  x [B][C][T] -> feat [B][n_bands][C][J].
 * Requires nperseg == 64, noverlap == 32 (the reference's STFT parameters). */
int isd_features_fused(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x,
                       float* feat, int64_t B, int64_t C, const int* klo, const int* khi,
                       int mode, float eps, void* stream);
/* The same with the feature map written as bf16: each value is the fp32 map's value rounded to nearest even.
 * BASELINE config 3: it is the rounding the bf16 classifier (isd_featcnn_step_bf16) and the reference's autocast apply
 * to the convolution's input anyway.  Both extractor families write it: the short-row one (nperseg 64 / noverlap 32,
 * rows of at most 1024 samples) and the long-row block-sum one (hop 64; the stress configuration, whose bf16 map the
 * EEGNet head reads through isd_eegnet_plan_set_input_dtype). */
int isd_features_fused_bf16(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x, uint16_t* feat,
                            int64_t B, int64_t C, const int* klo, const int* khi, int mode, float eps, void* stream);

/* Which kernel family the calling thread's last isd_features_fused / _bf16 call launched for its fp32 bands
 * (diagnostic; the tests that hold the two extractors against each other read it):
 *   0 none yet, 1 sixteen lanes per row (fused_kernel), 2 one row per lane (fused_serial_kernel: rows of whole
 *   32-sample chunks, bands of one or two bins; ISD_FUSED_SERIAL=0 in the environment selects 1), 3 the long-row
 *   block-sum kernels.
 * A plan without fp32 bands reports the family of its fp64 bands: 1 on short rows (fused_kernel), 3 on long rows. */
int isd_features_fused_last_path(void);
/* Within family 2: the waves per workgroup (16 or 8) if that call took the flat layout -- one band per wave, slots
 * numbered across workgroups; the default, with 8 waves, for three bands and more; ISD_SERIAL_FLAT=0 / 8 / 16 in the
 * environment overrides it -- and 0 after the grouped layout (ISD_SERIAL_BPW / ISD_SERIAL_GROUPS set, fewer bands) or any other
 * family. */
int isd_features_fused_last_serial_waves(void);

/* Input gradient of the extractor (spec S backward): dx = d<dfeat, feat(x)>/dx for the feature map that
 * isd_features_fused / isd_fb_forward + isd_stft_bandpower compute from x with the same plans, bins, mode and eps --
 * whichever kernel computed it.  The attributions of scripts/explain_fast.py / global_shap_analysis.py (gradients
 * w.r.t. the raw trials) through the feature classifiers.
 *   x [B][C][T] f32, dfeat [B][n_bands][C][J] f32, dx [B][C][T] f32 (overwritten).
 * Any STFT plan (power-of-two nperseg, any noverlap, ragged T), f32 / f64 / mixed filterbank plans, all three modes.
 * The filtered signals are recomputed per row and band, never materialised for the batch: `workspace` holds
 * isd_features_backward_workspace_bytes bytes (per-row scratch, bounded; larger batches run in row chunks).
 * Deterministic: no atomics, the bands are summed in a fixed order, and a trial's dx is the same at any batch size. */
int64_t isd_features_backward_workspace_bytes(const isd_fb_plan* fb, const isd_stft_plan* st, int64_t B, int64_t C,
                                              const int* klo, const int* khi);
int isd_features_backward(const isd_fb_plan* fb, const isd_stft_plan* st, const float* x, const float* dfeat,
                          float* dx, void* workspace, int64_t B, int64_t C, const int* klo, const int* khi,
                          int mode, float eps, void* stream);

/* ------------------------------------------------------------------------
 * Expected gradients (scripts/explain_fast.py, global_shap_analysis.py:
 *   shap.GradientExplainer(model, background).shap_values(X), local_smoothing = 0):
 *   phi_k[i] = (1/S) sum_s (x_i - b_r) * df_k/dx (b_r + alpha_is (x_i - b_r)),   r = ridx[i][s].
 * The two kernels are the sampling arithmetic around the model's forward and backward passes; the draws (ridx, alpha)
 * are made on the host (isd_amd.explain.draw_samples) and live on the device as [n][S] arrays.  A pair is
 * p = i * S + s; a TILE is the pairs pair0 .. pair0 + n_pairs - 1 and may start and end inside a trial.
 *   x [n][E] f32, bg [M][E] f32 (E = C*T elements per trial, any E >= 1: rows need dword alignment only),
 *   ridx [n*S] int32 in [0, M) -- checked by the caller, not here --, alpha [n*S] f32.
 * ---------------------------------------------------------------------- */
/* out [n_pairs][E]: out[q] = fmaf(alpha[p], x[p / S] - bg[ridx[p]], bg[ridx[p]]),  p = pair0 + q */
int isd_attr_mix(const float* x, const float* bg, const int32_t* ridx, const float* alpha, float* out,
                 int64_t n_pairs, int64_t pair0, int S, int64_t E, int M, void* stream);
/* grad [n_pairs][E]: the model's gradient at the tile's interpolated inputs; acc [n][E] (zeroed by the caller before
 * the first tile).  For every trial i with pairs in the tile and every element e, in s order within one thread,
 *   acc[i][e] = fmaf(x[i][e] - bg[ridx[p]][e], grad[p - pair0][e], acc[i][e]);
 * the difference is recomputed, never stored.  No atomics and no cross-lane sums: the bits do not depend on how the
 * pairs are cut into tiles, provided the tiles are passed in order.  A trial whose last pair (s = S - 1) lies in the
 * tile is multiplied by `scale` (1/S for the mean; 1 to keep the sum) after that pair, once. */
int isd_attr_accumulate(const float* x, const float* bg, const int32_t* ridx, const float* grad, float* acc,
                        int64_t n_pairs, int64_t pair0, int S, int64_t E, int M, float scale, void* stream);

/* ------------------------------------------------------------------------
 * Zero-phase FIR filter.  Replaces the band-pass of the SVM baseline,
 *   mne.filter.filter_data(X, 250, l_freq=4, h_freq=40)   notebooks/svm_baseline.ipynb:238-239, :968-969
 * (MNE is a third-party dependency that is not vendored in the reference; its documented defaults are restated:
 * method 'fir', fir_design 'firwin', hamming window, phase 'zero', pad 'reflect_limited').
 * taps: host, [n_taps] doubles, n_taps odd and symmetric (linear-phase type I); the host-side design lives in
 * isd_amd.filter_design.fir_design.  y[r][n] = sum_k taps[k] * xe[r][n - (n_taps-1)/2 + k] where xe is the row
 * extended by odd reflection about its end points over min(n_taps, T) - 1 samples and zeros beyond.
 * x, y [rows][T], distinct buffers.  _f32 computes in fp32, _f64 in fp64 (the notebook filters float64).
 * ---------------------------------------------------------------------- */
typedef struct isd_fir_plan isd_fir_plan;
int isd_fir_plan_create(isd_fir_plan** out, int n_taps, const double* taps);
int isd_fir_plan_destroy(isd_fir_plan* plan);
int isd_fir_plan_taps(const isd_fir_plan* plan);
int isd_fir_zero_phase_f32(const isd_fir_plan* plan, const float* x, float* y, int64_t rows, int T, void* stream);
int isd_fir_zero_phase_f64(const isd_fir_plan* plan, const double* x, double* y, int64_t rows, int T, void* stream);

/* ------------------------------------------------------------------------
 * Common Spatial Patterns: the data-sized steps of the transformer behind that band-pass,
 *   Pipeline(CSP(8, log=True) -> StandardScaler -> SVC)   notebooks/svm_baseline.ipynb:240-248, :307, :316
 * (mne.decoding.CSP; MNE is not vendored in the reference, its documented behaviour is restated).  The generalised
 * eigen-decomposition / joint diagonalisation of the [K][C][C] class covariances is host work: isd_amd.csp.decompose.
 * All pointers are device memory; no call synchronises with the host; 1 <= C <= 128, T >= 1.
 *
 * trial_cov:   x [n][C][T] -> cov [n][C][C], cov_i = X_i X_i^T / T: the second moment with no mean removal (MNE's
 *              empirical estimate for data assumed centred, reg=None).  cov[i][a][b] and cov[i][b][a] are the same
 *              bits.  The _f32 entry accumulates in fp32 on the fp32-input matrix cores, the _f64 entry in fp64.
 * group_mean:  cov [n][C][C] (fp64 when cov_f64 != 0, else fp32); idx [offs[K]] int64 trial indices in [0, n), grouped
 *              by class; offs [K+1] int64 with class k owning idx[offs[k] .. offs[k+1]); out [K][C][C] double,
 *              out_k = mean over the class's trials of cov_i, each divided by its trace first when norm_trace != 0
 *              (zeros for an empty class; NaN if an index lies outside [0, n)).  fp64 sums in the order of idx, one
 *              thread per element, no atomics: bitwise repeatable.
 * csp_power:   x [n][C][T], w [m][C] (1 <= m <= 16, same dtype) -> out [n][m],
 *              out[i][j] = mean_t (sum_c w[j][c] x[i][c][t])^2, its natural log when take_log != 0.  The projected
 *              signal is never written; the sum over T has a fixed order.
 * ---------------------------------------------------------------------- */
int isd_trial_cov_f32(const float* x, float* cov, int64_t n, int C, int T, void* stream);
int isd_trial_cov_f64(const double* x, double* cov, int64_t n, int C, int T, void* stream);
int isd_cov_group_mean(const void* cov, int cov_f64, const int64_t* idx, const int64_t* offs, int norm_trace,
                       double* out, int64_t n, int C, int K, void* stream);
int isd_csp_power_f32(const float* x, const float* w, float* out, int64_t n, int C, int T, int m, int take_log,
                      void* stream);
int isd_csp_power_f64(const double* x, const double* w, double* out, int64_t n, int C, int T, int m, int take_log,
                      void* stream);

/* ------------------------------------------------------------------------
 * Filter-bank CSP (Ang et al. 2008; isd_amd.FBCSP): the two steps above for every band of a filterbank plan, without
 * the filtered [n][n_bands][C][T] map in memory.  Any plan of isd_fb_plan_create is taken (<= 8 sections, F32 / F64 /
 * AUTO, mixed sets); bands come out in the caller's order.  All pointers are device memory; no call synchronises with
 * the host; n == 0 returns 0 without a launch; 1 <= C <= 128, T >= 1.  A trial's result depends on the plan, C, T and
 * m only, never on n or on its position in the batch, and is the same bits on every call.
 *
 * fb_trial_cov: x [n][C][T] f32 -> cov [n][n_bands][C][C] f32,
 *               cov[i][b] = Y Y^T / T with Y = gain_b * cascade_b(x_i): causal, zero initial state, samples 0 .. T-1
 *               only.  No mean removal.  [a][c] and [c][a] are the same bits.
 * fb_csp_power: w [n_bands][m][C] f32 (1 <= m <= 16) -> out [n][n_bands][m] f32,
 *               out[i][b][j] = mean_{t<T} (gain_b * cascade_b(sum_c w[b][j][c] x_i[c][.]))[t]^2, its natural log when
 *               take_log != 0.  The projection is formed first, then filtered; the sum over T has a fixed order.
 * ---------------------------------------------------------------------- */
int isd_fb_trial_cov(const isd_fb_plan* plan, const float* x, float* cov, int64_t n, int C, int T, void* stream);
int isd_fb_csp_power(const isd_fb_plan* plan, const float* x, const float* w, float* out, int64_t n, int C, int T,
                     int m, int take_log, void* stream);

/* ------------------------------------------------------------------------
 * Independent component analysis: the data-sized steps of parallel FastICA with the logcosh contrast (alpha = 1), the
 * default method of the reference's artifact removal
 *   ICA(n_components, method='fastica').fit(epochs); ica.apply(epochs)   scripts/artifact_analysis.py:61
 * (mne.preprocessing.ICA -> sklearn.decomposition.FastICA).  Centring, whitening and the symmetric decorrelation work
 * on [m][C] matrices and are host work: isd_amd.ica.fastica.  All pointers are device memory; no call synchronises
 * with the host; 1 <= C <= 128, T >= 1.
 *
 * ica_step:       x [n][C][T], U [m][C], b [m] (1 <= m <= 64, same dtype) -> P [m][C], s [m], q [m], all double:
 *                 with G_i = tanh(U x_i - b) per sample,  P = sum_i G_i x_i^T,  s = sum G,  q = sum (1 - G^2), over
 *                 all n * T samples.  One pass over x; neither the projection nor G is written.  The _f32 entry does
 *                 the per-sample arithmetic and each workgroup's partial sums in fp32 on the fp32-input matrix cores,
 *                 the _f64 entry in fp64; the partials are then added in fp64 in a fixed order (no atomics): bitwise
 *                 repeatable.  `work`: isd_ica_step_work_bytes(n, C, T, m, is_f64) bytes of scratch (-1 on a bad shape).
 * spatial_apply:  x [n][C][T], M [R][C] (1 <= R <= 128), bias [R] or NULL -> out [n][R][T],
 *                 out_i = M x_i + bias[:, None].  out must not overlap x.
 * ---------------------------------------------------------------------- */
int64_t isd_ica_step_work_bytes(int64_t n, int C, int T, int m, int is_f64);
int isd_ica_step_f32(const float* x, const float* U, const float* b, double* P, double* s, double* q, void* work,
                     int64_t work_bytes, int64_t n, int C, int T, int m, void* stream);
int isd_ica_step_f64(const double* x, const double* U, const double* b, double* P, double* s, double* q, void* work,
                     int64_t work_bytes, int64_t n, int C, int T, int m, void* stream);
int isd_spatial_apply_f32(const float* x, const float* M, const float* bias, float* out, int64_t n, int C, int T,
                          int R, void* stream);
int isd_spatial_apply_f64(const double* x, const double* M, const double* bias, double* out, int64_t n, int C, int T,
                          int R, void* stream);

/* ------------------------------------------------------------------------
 * Riemannian geometry of covariance matrices (isd_amd.riemann: Covariances -> TangentSpace -> a linear classifier, and
 * MDM, Barachant et al. 2012; pyriemann is not vendored in the reference, the published method is restated): matrix
 * functions of n small symmetric positive-definite matrices behind isd_trial_cov_*.  All arithmetic is fp64.  The
 * square roots, exp and step control of the [K][C][C] class means are host work: isd_amd.riemann.mean_riemann.
 * All pointers are device memory; no call synchronises with the host, takes a workspace or uses atomics; n == 0 returns
 * 0 without a launch; 1 <= C <= 128, beyond that ISD_ERR_UNSUPPORTED.  A matrix's result depends on that matrix (and
 * its W) alone, never on n, its position or an earlier launch, and is the same bits on every call.
 *
 * spd_congruence: cov [n][C][C] (fp64 when cov_f64 != 0, else fp32: what isd_trial_cov_* leave), W [K][C][C] double,
 *                 widx [n] int32 in [0, K) or NULL (then W[0] for all) -> out [n][C][C] double,
 *                 out_i = W_k cov_i W_k^T with k = widx[i].  Only the upper triangle of the second product is formed
 *                 (as if cov_i were symmetric); out[i][a][b] and out[i][b][a] are the same bits.  A matrix whose
 *                 widx lies outside [0, K) comes out NaN.  out must not be cov or W.
 * spd_eigfun:     a [n][C][C] double, symmetric positive (semi-)definite -> with A = V L V^T:  f(A) = V f(L) V^T,
 *                 f = log, sqrt, 1/sqrt, 1/x or x for fn = ISD_SPD_LOG .. ISD_SPD_NONE.
 *                 out_kind ISD_SPD_FULL:    out [n][C][C], [a][b] and [b][a] the same bits;
 *                          ISD_SPD_TANGENT: out [n][C(C+1)/2], the upper triangle row by row (np.triu_indices(C)
 *                                           order) with the off-diagonal entries times sqrt 2, whose Euclidean norm
 *                                           is the Frobenius norm of f(A);
 *                          ISD_SPD_NOOUT:   nothing, out may be NULL.
 *                 eigvals [n][C] or NULL: the eigenvalues in no promised order.
 *                 info [n] int32 or NULL: the number of Jacobi sweeps used (> 0);  -1 if the cap of 30 sweeps was
 *                 reached (out then holds the unconverged result);  -2 if an eigenvalue is not finite, the matrix is
 *                 indefinite, or fn is log, 1/sqrt or 1/x and an eigenvalue is <= 0: that matrix's out is then NaN.
 *                 One-sided Jacobi on A itself: like LAPACK's eigh it resolves an eigenvalue to about
 *                 eps * l_max absolute, so log and the inverses of a matrix of condition k carry about eps * k.
 *                 Only the magnitudes of the eigenvalues survive the iteration; a negative one is detected through
 *                 trace(A) < sum |l_j| (1 - 64 C eps), so one below that share of the trace is taken by magnitude.
 *                 out must not be a.
 * ---------------------------------------------------------------------- */
enum { ISD_SPD_LOG = 0, ISD_SPD_SQRT = 1, ISD_SPD_INVSQRT = 2, ISD_SPD_INV = 3, ISD_SPD_NONE = 4 };
enum { ISD_SPD_FULL = 0, ISD_SPD_TANGENT = 1, ISD_SPD_NOOUT = 2 };
int isd_spd_congruence(const void* cov, int cov_f64, const double* W, const int32_t* widx, double* out, int64_t n,
                       int C, int K, void* stream);
int isd_spd_eigfun(const double* a, double* out, double* eigvals, int32_t* info, int64_t n, int C, int fn,
                   int out_kind, void* stream);

/* ------------------------------------------------------------------------
 * Welch power spectral density: the data-sized step of
 *   raw.compute_psd(method='welch') -> mne.time_frequency.psd_array_welch   scripts/artifact_analysis.py:45
 * as scipy.signal.welch / spectrogram(scaling='density') compute it.  Segment s of a row is samples
 * s * step .. s * step + n_per_seg - 1 (step = n_per_seg - n_overlap), S = (T - n_per_seg) / step + 1 whole segments,
 * no boundary extension; samples after the last whole segment are not read.  Each segment has its mean removed (if
 * remove_dc), is multiplied by `window` [n_per_seg] (host, double), zero-padded to n_fft, and the one-sided power of
 * bins k_lo .. k_hi is scaled to a density:  |X_k|^2 c_k / (sfreq sum w^2),  c_k = 2 except 1 at k = 0 and at
 * k = n_fft / 2 for even n_fft.  The transform is a dense product with a windowed cos / sin table the plan owns (one
 * copy per precision): only the kept bins cost arithmetic.
 *
 * x [rows][T] -> out [rows][K] the mean over segments, or with per_segment != 0 out [rows][K][S]; K = k_hi - k_lo + 1.
 * The _f32 entry multiplies and accumulates in fp32 on the fp32-input matrix cores, the _f64 entry in fp64; the
 * segment means are taken in fp64 in both.  `work`: isd_psd_work_bytes bytes of scratch.  Sums run in segment order
 * with no atomics: bitwise repeatable.  x needs element alignment only.  All data pointers are device memory; no call
 * synchronises with the host.
 * Envelope: 2 <= n_fft <= 2048, 1 <= n_per_seg <= n_fft, 0 <= n_overlap < n_per_seg, 0 <= k_lo <= k_hi <= n_fft / 2,
 * T >= n_per_seg, any rows >= 0 (rows = 0 returns at once); outside it ISD_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------- */
typedef struct isd_psd_plan isd_psd_plan;
int isd_psd_plan_create(isd_psd_plan** out, int n_fft, int n_per_seg, int n_overlap, int k_lo, int k_hi,
                        const double* window /* host [n_per_seg] */, double sfreq, int remove_dc);
int isd_psd_plan_destroy(isd_psd_plan* plan);
int isd_psd_plan_bins(const isd_psd_plan* plan);                    /* K */
int64_t isd_psd_plan_segments(const isd_psd_plan* plan, int64_t T); /* S, 0 if T < n_per_seg */
/* exactly what the launch addresses: the fp64 segment means, then each z's partial spectra in whole 256-byte lines when
 * the segments are split over z, one line of slack when they are not (256 for rows == 0 or T < n_per_seg) */
int64_t isd_psd_work_bytes(const isd_psd_plan* plan, int64_t rows, int64_t T, int is_f64);
int isd_psd_welch_f32(const isd_psd_plan* plan, const float* x, float* out, int64_t rows, int64_t T, int per_segment,
                      void* work, void* stream);
int isd_psd_welch_f64(const isd_psd_plan* plan, const double* x, double* out, int64_t rows, int64_t T, int per_segment,
                      void* work, void* stream);

/* ------------------------------------------------------------------------
 * Cross-spectral density by Welch's method on a Welch PSD plan: its segments, window, kept bins, scale and remove_dc.
 *   S[k][i][j] = scale[k] / N  sum X_i[k] conj(X_j[k]),   X[k] = sum_t (x[t] - mean) w[t] exp(-2 pi i k t / n_fft),
 * which is scipy.signal.csd(x_j, x_i, detrend='constant', scaling='density') (scipy conjugates its first argument).
 * x [n][C][T] -> out complex, (re, im) interleaved:  over_trials == 0: [n][K][C][C][2], the sum over the S segments of
 * a trial, N = S;  over_trials != 0: [K][C][C][2], the sum over every (trial, segment), N = n S.  With unit_modulus
 * every X[k] is first divided by its modulus (an exact zero stays zero) and the factor is 1 / N: the mean phase
 * difference behind the phase-locking measures.  out[.., i, j] is the exact conjugate of out[.., j, i] and the
 * diagonal's imaginary part is exactly 0.  Sums run in (trial, segment) order with no atomics: bitwise repeatable.
 * `work`: isd_csd_work_bytes bytes, 256-byte aligned; it is bounded: the trials run in chunks inside the call, of
 * at most isd_csd_chunk_bytes of intermediate spectra each (default 256 MiB; isd_csd_chunk_bytes(b) sets it for
 * later calls of the calling thread, b = 0 restores the default, b < 0 only asks; returns the value before), and over_trials adds the
 * chunks in order.  x needs element alignment only, out that of one complex element.  No call synchronises with the
 * host.  Envelope: the plan's, 1 <= C <= 128, T >= n_per_seg, n >= 0 (n = 0 returns at once); outside it
 * ISD_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------- */
int64_t isd_csd_chunk_bytes(int64_t bytes);
/* exactly what the launch addresses (means, one chunk's spectra, with over_trials the range sums and the accumulator,
 * each from a 256-byte line) plus one line of slack: never 0 */
int64_t isd_csd_work_bytes(const isd_psd_plan* plan, int64_t n, int64_t C, int64_t T, int over_trials, int is_f64);
int isd_csd_welch_f32(const isd_psd_plan* plan, const float* x, float* out, int64_t n, int64_t C, int64_t T,
                      int over_trials, int unit_modulus, void* work, void* stream);
int isd_csd_welch_f64(const isd_psd_plan* plan, const double* x, double* out, int64_t n, int64_t C, int64_t T,
                      int over_trials, int unit_modulus, void* work, void* stream);

/* ------------------------------------------------------------------------
 * Pairwise envelope correlation (csrc/envcorr.hip; isd_amd.connectivity.envelope_correlation).  z [n][C][T][2] is the
 * analytic signal of n trials, (re, im) interleaved; out [n][C][C] real.  Per trial, with m = |z|, e = m (flag 1:
 * log m^2), ec = e - mean_t e and se = |ec|_2 (1 where it is 0):
 *   orthogonalised (flag 4 clear): o[l|j] = |Im(z_l conj(z_j))| / m_j (0 where m_j = 0; flag 1: log o^2), centred over
 *     t, correlated with ec_j: corr[l|j] = sum_t oc ec_j / (se_j |oc|_2) (|oc|_2 = 1 where it is 0);
 *     out[l][j] = out[j][l] = (A[l|j] + A[j|l]) / 2 with A = |corr| under flag 2, else corr; the diagonal is 0.
 *   plain (flag 4): out[l][j] = sum_t ec_l ec_j / (se_l se_j); the diagonal is 1, or 0 for a row of zero norm;
 *     flag 2 is ignored.
 * Sums over t are fp64 in both precisions, in sample order, with no atomics: bitwise repeatable, and out is symmetric
 * bit for bit.  With flag 1 an exact zero of m or o makes the entries it enters NaN and no other.
 * `work`: isd_envcorr_work_bytes bytes (about the size of z), 256-byte aligned.  z and out need the alignment of one
 * complex / one real element.  No call synchronises with the host.  n == 0 returns 0 with nothing touched;
 * C outside 1..128 is ISD_ERR_UNSUPPORTED; a null pointer, T < 1 with n > 0 or an unknown flag is ISD_ERR_INVALID.
 * ---------------------------------------------------------------------- */
/* exactly what the launch addresses (row statistics, then W from a 256-byte line) plus 256 bytes of slack: never 0;
 * negative = error code */
int64_t isd_envcorr_work_bytes(int64_t n, int64_t C, int64_t T, int is_f64);
int isd_envcorr_f32(const float* z /* [n][C][T][2] */, float* out /* [n][C][C] */, int64_t n, int64_t C, int64_t T,
                    int flags /* 1 log | 2 absolute | 4 plain */, void* work, void* stream);
int isd_envcorr_f64(const double* z, double* out, int64_t n, int64_t C, int64_t T, int flags, void* work,
                    void* stream);

/* ------------------------------------------------------------------------
 * Time-resolved spectral connectivity (csrc/contime.hip; isd_amd.connectivity.spectral_connectivity_time).
 * z [n][C][F][T_out][2] is the complex wavelet map of n trials, (re, im) interleaved (isd_tfr_cwt_*, mode 0); the
 * samples t0 <= t < t1 are averaged, N = t1 - t0.  Per (trial, frequency, channels i, j), s = w_i conj(w_j),
 * u = s / |s| (0 where |s| = 0; formed as u_i conj(u_j) from each channel's w / |w|), <.> the mean over the samples:
 *   bit 0 coh    |<s>| / sqrt(<|w_i|^2> <|w_j|^2>)          bit 4 pli    |<sign Im s>|
 *   bit 1 imcoh  Im <s> / sqrt(<|w_i|^2> <|w_j|^2>)         bit 5 dpli   <H(Im s)>, H(0) = 1/2
 *   bit 2 plv    |<u>|                                      bit 6 wpli   |<Im s>| / <|Im s|>
 *   bit 3 ciplv  |Im <u>| / sqrt((1 - |Re <u>|)(1 + |Re <u>|))
 *   bit 7 wpli2_debiased  ((sum Im s)^2 - sum (Im s)^2) / ((sum |Im s|)^2 - sum (Im s)^2)
 * out real, the M measures of methods_mask in bit order: average == 0: [M][n][F][C][C]; average != 0: [M][F][C][C],
 * the mean over the n trials of the per-trial measure, added in fp64 in trial order by the one wave that owns the
 * (frequency, tile pair): no workspace, and F x (tile pairs) waves of parallelism only.  Im s is a compensated cross
 * product (its sign is that of the exact Im s of the stored values unless |Im s| is below about 2^-47 |w_i| |w_j|
 * in fp32, 2^-105 in fp64, where a plain difference of two products loses it at 2^-24 / 2^-53); every sum over t is fp64 or
 * an integer count, in sample order, with no atomics: bitwise repeatable.  Both triangles are written: the same bits
 * for the six symmetric measures, out[j][i] = -out[i][j] (imcoh) and 1 - out[i][j] (dpli) in the output's arithmetic
 * for i > j.  The diagonal is set, not computed: 1 (coh, plv), 0 (imcoh, pli), 1/2 (dpli), NaN (ciplv, wpli,
 * wpli2_debiased: 0 / 0).  A channel that is zero over [t0, t1) gives, off the diagonal of its row and column, NaN
 * for coh, imcoh, wpli and wpli2_debiased, 0 for plv, ciplv and pli and 1/2 for dpli, and changes no other entry.
 * z and out need the alignment of one complex / one real element.  No call synchronises with the host.  n == 0
 * returns 0 with nothing touched (ISD_ERR_INVALID with average); C outside 1..128 is ISD_ERR_UNSUPPORTED; a null
 * pointer, an empty or unknown methods_mask, F < 1 or not 0 <= t0 < t1 <= T_out is ISD_ERR_INVALID.
 * ---------------------------------------------------------------------- */
int isd_contime_f32(const float* z /* [n][C][F][T_out][2] */, float* out, int64_t n, int64_t C, int64_t F,
                    int64_t T_out, int64_t t0, int64_t t1, int methods_mask, int average, void* stream);
int isd_contime_f64(const double* z, double* out, int64_t n, int64_t C, int64_t F, int64_t T_out, int64_t t0,
                    int64_t t1, int methods_mask, int average, void* stream);

/* ------------------------------------------------------------------------
 * Phase-amplitude coupling with circular-shift surrogates (csrc/pac.hip; isd_amd.phase_amplitude_coupling).
 * pha [rows][P][T] phases in [-pi, pi], amp [rows][A][T] amplitudes >= 0, shifts int32 [1 + S] on the device with
 * shifts[0] = 0 (the estimate) and 0 <= shifts[i] < T (the surrogates: amp read at (t + shift) mod T).  The phase bin
 * is min(n_bins - 1, max(0, floor((double(pha) + pi) * c))), c = n_bins / (2 pi) formed by the caller, in fp64 in both
 * entries.  out [rows][A][P][3][4]: per method (0 mean vector length, 1 modulation index, 2 heights ratio) the value
 * at shift 0, the mean and the population std of the S surrogate values (fp64 sums of the values as rounded to the
 * output type) and the number of surrogates >= the value.  surr, if not null, [rows][A][P][3][S]: every surrogate
 * value.  With S = 0 mean and std are NaN and the count is 0.  Every sum runs in a fixed order with no atomics: bitwise
 * repeatable.  A shift outside [0, T - 1] is clamped, and shift 0 is read as 0.
 * `work`: isd_pac_work_bytes bytes (the bin-sorted (cos, sin, t) records of pha: 3 x its size in fp32, 2.5 x in fp64),
 * 256-byte aligned; every array needs its element's alignment.  No call synchronises with the host.  rows == 0 returns
 * 0 with nothing touched.  Envelope: 1 <= T <= 4096, 2 <= n_bins <= 64, 0 <= S <= 4095, P, A >= 1,
 * rows * A * P < 2^31; outside it ISD_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------- */
/* exactly what the launch addresses (ranked records, sample indices, bin offsets, the surrogates' order, each from a
 * 256-byte line; the last is there for rows == 0 too: never 0); negative = error code */
int64_t isd_pac_work_bytes(int64_t rows, int64_t P, int64_t A, int64_t T, int is_f64);
int isd_pac_f32(const float* pha, const float* amp, const int32_t* shifts, float* out, float* surr, int64_t rows,
                int64_t P, int64_t A, int64_t T, int64_t S, int n_bins, double c, void* work, void* stream);
int isd_pac_f64(const double* pha, const double* amp, const int32_t* shifts, double* out, double* surr, int64_t rows,
                int64_t P, int64_t A, int64_t T, int64_t S, int n_bins, double c, void* work, void* stream);

/* ------------------------------------------------------------------------
 * Complex FIR bank with decimation: the data-sized step of a time-frequency transform
 * (isd_amd.tfr_array_morlet, the counterpart of mne.time_frequency.tfr_array_morlet; isd_amd.tfr.cwt).  The library
 * knows nothing about wavelets: the plan takes n_freqs complex tap vectors of odd lengths and
 *   z[row][f][t] = sum_k w_f[k] x[row][t decim + h_f - k],   h_f = (n_taps[f] - 1) / 2,   x zero outside [0, T),
 * which is np.convolve(x[row], w_f, 'same')[::decim]; T_out = ceil(T / decim) (isd_tfr_plan_out_len).  Only kept
 * samples are computed.  The product runs on the fp32 / fp64 matrix cores with eight frequencies x (re, im) side by
 * side, the taps of a group of eight (sorted by length) centred and zero-padded to the longest: useful and padded
 * tap counts differ by isd_tfr_plan_padded_taps / sum(n_taps).
 *
 * x [n][C][T] -> out by `mode`:
 *   0  complex    [n][C][F][T_out][2]  (re, im)
 *   1  power      [n][C][F][T_out]     re^2 + im^2
 *   2  avg_power  [C][F][T_out]        mean over the n trials of the power
 *   3  itc        [C][F][T_out]        | mean over trials of z / |z| |; a sample with |z| = 0 contributes 0
 *   4  both       [C][F][T_out][2]     (avg_power, itc), the same bits as modes 2 and 3
 *   5  phase      [n][C][F][T_out]     atan2(im, re), taken in fp64
 * The _f32 entry multiplies and accumulates in fp32, the _f64 entry in fp64, out has x's type; the exceptions are the
 * phase and the coherence of the _f32 entry (modes 5, 3 and the second half of mode 4), whose product runs in fp64
 * over the widened samples, because the phase of a weak sample does not survive fp32 (mode 4 then costs modes
 * 2 + 3).  Modes 2-4 write
 * nothing per trial: the owner of an output element walks the trials in index order, sums in fp64 in both entries and
 * stores once.  No atomics: every mode is bitwise repeatable.  Each row's mean (fp64, a pre-pass into `work`) is taken
 * off before the product and its share, mean x the sum of the taps that met the row, is added back in fp64: the
 * result is the same and an offset of the data costs no precision.  `work`: isd_tfr_work_bytes bytes of scratch (the
 * n C means).  x needs element alignment only; out the alignment of its element, which for modes 0 and 4 is the (re, im)
 * pair.  All data pointers are device memory; taps and n_taps are host memory; no call synchronises with the host.
 * Envelope: 1 <= n_freqs <= 256, odd 1 <= n_taps <= 4095, 1 <= decim <= 128, finite taps, any n, C, T >= 0 with
 * n, C < 2^31 (an empty array returns at once, but n = 0 with modes 2-4 is ISD_ERR_INVALID), at most 2^31 - 1
 * (row, time tile) pairs; outside it ISD_ERR_UNSUPPORTED with the reason in isd_last_error().
 * ---------------------------------------------------------------------- */
typedef struct isd_tfr_plan isd_tfr_plan;
int isd_tfr_plan_create(isd_tfr_plan** out, int n_freqs, const int* n_taps /* host [F], odd */,
                        const double* taps /* host, (re, im) pairs, sum(n_taps) of them */, int decim);
int isd_tfr_plan_destroy(isd_tfr_plan* plan);
int64_t isd_tfr_plan_out_len(const isd_tfr_plan* plan, int64_t T);   /* ceil(T / decim) */
int64_t isd_tfr_plan_padded_taps(const isd_tfr_plan* plan);          /* taps multiplied per output column, zeros included */
int64_t isd_tfr_work_bytes(const isd_tfr_plan* plan, int64_t n, int64_t C, int64_t T, int mode, int is_f64);
int isd_tfr_cwt_f32(const isd_tfr_plan* plan, const float* x, void* out, int64_t n, int64_t C, int64_t T, int mode,
                    void* work, void* stream);
int isd_tfr_cwt_f64(const isd_tfr_plan* plan, const double* x, void* out, int64_t n, int64_t C, int64_t T, int mode,
                    void* work, void* stream);

/* ------------------------------------------------------------------------
 * Polyphase rational resampling of rows: scipy.signal.resample_poly (isd_amd.resample_poly, isd_amd.resample).
 *   y[row][n] = bg + sum_m xe[m] h[half_len + n down - m up]   over the m with 0 <= half_len + n down - m up < n_taps,
 *   0 <= n < n_out = ceil(T up / down)  (isd_resample_out_len),
 * xe the row minus bg extended beyond 0 .. T-1 by `mode`: ISD_RESAMPLE_CONSTANT the value cval, _EDGE the end
 * samples, _REFLECT the whole-sample mirror (period 2T - 2), _SYMMETRIC the half-sample mirror (period 2T), _LINE the
 * straight line through x[0] and x[T-1].  bg = background[row] (device, fp64) or 0 when background is NULL; it is
 * taken off in fp64 while the row is read and added back to y, which is how the host provides scipy's 'mean',
 * 'median', 'minimum' and 'maximum' pad types (mode _CONSTANT, cval 0).  The library designs no filter: the plan takes
 * up / down already reduced by their gcd, and the taps (host, fp64) already multiplied by up, with their centre.
 *
 * x [rows][T] -> y [rows][n_out], distinct buffers, element alignment only.  _f32 computes on the fp32 matrix cores,
 * _f64 on the fp64 ones; no atomics, a row's result does not depend on the other rows of the call, and a sample
 * outside 0 .. T-1 is never read.  Within a row an infinite sample reaches the up to 15 neighbouring outputs of its
 * block of 16 through a zero tap (inf . 0), which scipy's loop would skip.  No call synchronises with the host.
 *
 * Envelope: up, down <= ISD_RESAMPLE_MAX_RATE, n_taps <= ISD_RESAMPLE_MAX_TAPS, device tables within 16 MiB,
 * n_out < 2^31, T >= 1 (T >= 2 for _REFLECT and _LINE: ISD_ERR_INVALID); outside it ISD_ERR_UNSUPPORTED with the
 * reason in the last-error string.
 * ---------------------------------------------------------------------- */
enum { ISD_RESAMPLE_CONSTANT = 0, ISD_RESAMPLE_EDGE = 1, ISD_RESAMPLE_REFLECT = 2, ISD_RESAMPLE_SYMMETRIC = 3,
       ISD_RESAMPLE_LINE = 4 };
enum { ISD_RESAMPLE_MAX_RATE = 1024, ISD_RESAMPLE_MAX_TAPS = 20481 };
typedef struct isd_resample_plan isd_resample_plan;
int isd_resample_plan_create(isd_resample_plan** out, int up, int down, int n_taps, const double* taps /* host */,
                             int half_len);
int isd_resample_plan_destroy(isd_resample_plan* plan);
int64_t isd_resample_out_len(const isd_resample_plan* plan, int64_t T);
int isd_resample_poly_f32(const isd_resample_plan* plan, const float* x, float* y, int64_t rows, int T, int mode,
                          double cval, const double* background /* device [rows] or NULL */, void* stream);
int isd_resample_poly_f64(const isd_resample_plan* plan, const double* x, double* y, int64_t rows, int T, int mode,
                          double cval, const double* background /* device [rows] or NULL */, void* stream);

/* ------------------------------------------------------------------------
 * Zone-wise Conv4Layers stack over sliding windows: the reference's
 *   FAST.forward_head   src/fast/models/fast.py:242-252  (unfold window_len / slide_step)
 *   Head.forward        src/fast/models/fast.py:209-210  (zone gather, one encoder per zone, stack)
 *   Conv4Layers.forward src/fast/models/fast.py:111-119  (cnn1..cnn4, exact GELU, mean over time)
 * x [B][c_total][T] f32 -> feat [B*N][n_zones][F] f32 (== the reference's [B, N, Z, F]),
 * N = (T - window_len) / slide_step + 1.  The spec-S feature classifier uses the same
 * entry points with one zone of nb*C "channels" and window_len == T == J.
 *
 * Parameters live in ONE flat f32 block (so that data-parallel training
 * all-reduces a single bucket): per zone, in the reference's state_dict order,
 *   cnn1.weight [F,1,1,5] | cnn1.bias [F] | cnn2.weight [F,F,Cz,1] | cnn3.weight [F,F,1,5] | cnn4.weight [F,F,1,5]
 * (n_layers == 2 drops cnn3/cnn4: the build-defined "2-layer CNN" of BASELINE config 1).
 * ---------------------------------------------------------------------- */
typedef struct isd_conv4_plan isd_conv4_plan;

/* zone_sizes: host [n_zones]; zone_channels: host, concatenated channel indices (Head.index_dict, fast.py:206) */
int isd_conv4_plan_create(isd_conv4_plan** out, int c_total, int n_zones, const int* zone_sizes,
                          const int* zone_channels, int feature_dim, int n_layers, int window_len,
                          int slide_step);
int isd_conv4_plan_destroy(isd_conv4_plan* plan);
/* BASELINE config 3: ISD_ACT_BF16 stores activations and activation gradients as bf16 and rounds the staged
 * operands (inputs, weights) to bf16, accumulating in fp32 -- the arithmetic of bf16-mixed autocast
 * (scripts/train_fast.py:277).  Parameters, parameter gradients, features and the FC head stay fp32. */
enum { ISD_ACT_F32 = 0, ISD_ACT_BF16 = 1 };
int isd_conv4_plan_set_activation_dtype(isd_conv4_plan* plan, int dtype);
int64_t isd_conv4_param_count(const isd_conv4_plan* plan);
/* which: 0 cnn1.weight, 1 cnn1.bias, 2 cnn2.weight, 3 cnn3.weight, 4 cnn4.weight -> offset in floats */
int64_t isd_conv4_param_offset(const isd_conv4_plan* plan, int zone, int which);
int isd_conv4_windows(const isd_conv4_plan* plan, int64_t T);
/* exactly what the calls on this plan address at (B, T), in whole 256-byte lines; every route's slabs fit the last region */
int64_t isd_conv4_workspace_bytes(const isd_conv4_plan* plan, int64_t B, int64_t T);

/* forward keeps the activations the backward needs inside `workspace` (caller-owned,
 * isd_conv4_workspace_bytes bytes); backward must see the same x, params and workspace.
 * dparams: flat gradient block, same layout as params, overwritten. */
int isd_conv4_forward(const isd_conv4_plan* plan, const float* x, const float* params, float* feat,
                      void* workspace, int64_t B, int64_t T, void* stream);
int isd_conv4_backward(const isd_conv4_plan* plan, const float* x, const float* params,
                       const float* dfeat, float* dparams, void* workspace, int64_t B, int64_t T,
                       void* stream);
/* As isd_conv4_backward, and additionally dx [B][c_total][T] = dL/dx (zeroed here, then accumulated over zones and
 * overlapping windows).  Takes the layer-wise backward (the fused one keeps the activation gradients in LDS); fp32
 * activations only.  Off the hot path: it serves input attributions (scripts/explain_fast.py,
 * scripts/global_shap_analysis.py differentiate the model w.r.t. its input). */
int isd_conv4_backward_x(const isd_conv4_plan* plan, const float* x, const float* params, const float* dfeat,
                         float* dparams, float* dx, void* workspace, int64_t B, int64_t T, void* stream);

/* ------------------------------------------------------------------------
 * Dense head on the matrix cores (fp32-in MFMA).  nn.Linear semantics:
 *   y[M][N] = act(x[M][K] . w[N][K]^T + bias[N]),  act: 0 none, 1 exact-erf GELU.
 * Replaces FAST.input_layer (Linear 256->32 + GELU, fast.py:235) and
 * FAST.last_layer (Linear 32->5, fast.py:239) as used at fast.py:276-277.
 * `pre` (nullable) receives the pre-activation, which backward needs when act == 1.
 * ---------------------------------------------------------------------- */
int isd_linear_forward(const float* x, const float* w, const float* bias, float* y, float* pre,
                       int64_t M, int K, int N, int act, void* stream);
/* y = x . w^T + bias + res   (residual connection fused in the epilogue; fast.py:24-25) */
int isd_linear_residual_forward(const float* x, const float* w, const float* bias, const float* res, float* y,
                                int64_t M, int K, int N, void* stream);
/* isd_linear_backward's workspace: 4 (M N + slabs N (K + 1) + 64) bytes -- exactly the activation gradient, the weight
 * gradient slabs from the next 256-byte line, and what is left of the 64 floats as slack */
int64_t isd_linear_workspace_bytes(int64_t M, int K, int N);
/* dx nullable; db nullable */
int isd_linear_backward(const float* x, const float* w, const float* dy, const float* pre, float* dx,
                        float* dw, float* db, void* workspace, int64_t M, int K, int N, int act,
                        void* stream);

/* ------------------------------------------------------------------------
 * Token mean + softmax cross-entropy + argmax:
 *   logits = logits_tok.mean(dim=1)                         fast.py:277
 *   loss   = nn.CrossEntropyLoss()(logits, y)               trainer.py:37,59  (mean; uint8 or int64 labels)
 *   pred   = argmax(logits, dim=1), ties -> lowest index    trainer.py:89
 * logits_tok [B][n_tok][n_cls]; grad_scale = 1 / global batch size (1/B on one GPU);
 * loss receives grad_scale * sum_b CE_b; dlogits_tok gets d loss / d logits_tok.
 * labels == NULL: inference (no loss / gradient).  Any output pointer may be NULL.
 * workspace: isd_softmax_ce_workspace_bytes(B) bytes of scratch (per-block partial sums + an
 * arrival ticket; contents need not be initialised); only needed when the loss is requested.
 * ---------------------------------------------------------------------- */
/* exactly what the launch addresses: the ticket's 256-byte line, then one float per 256 trials */
int64_t isd_softmax_ce_workspace_bytes(int64_t B);
int isd_softmax_ce(const float* logits_tok, const void* labels, int label_bytes, float* logits_mean,
                   float* loss, float* dlogits_tok, int64_t* pred, int64_t B, int n_tok, int n_cls,
                   float grad_scale, void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * EEGNet_Encoder (src/fast/models/fast.py:122-167): the "EEGNet-style depthwise CNN" head.
 *   x [B][C][T] f32 -> out [B][feature_dim];  kernel_length even, <= 64 (reference default 64).
 * Flat parameter block (reference state_dict order, trainable tensors only):
 *   temporal_conv.0.weight [8,1,1,K] | temporal_conv.1.weight [8] | .bias [8] | spatial_conv.0.weight [16,1,C,1] |
 *   spatial_conv.1.weight [16] | .bias [16] | separable_conv.0.weight [16,1,1,16] | separable_conv.1.weight [16,16,1,1] |
 *   separable_conv.2.weight [16] | .bias [16] | projector.2.weight [F,16] | projector.2.bias [F]
 * Buffer block (80 floats): running_mean/var of BN1 (8,8), BN2 (16,16), BN3 (16,16); updated in place when training.
 * training != 0: batch statistics (biased variance for the normalisation, unbiased for the running update);
 * dropout_p (train only) uses a counter-based mask keyed by `seed` (pass the same p and seed to backward): it is
 * statistically, not bitwise, nn.Dropout.  The temporal-conv activation [B,8,C,T+1] is never formed.
 * backward: parameter gradients only (x is data); one backward per forward, same workspace.
 * ---------------------------------------------------------------------- */
typedef struct isd_eegnet_plan isd_eegnet_plan;
int isd_eegnet_plan_create(isd_eegnet_plan** out, int in_channels, int feature_dim, int kernel_length, int T);
/* CVBlock (src/fast/models/fast.py:32-100): the same plan type and the same isd_eegnet_* entry points below, with
 * stage 1 pooled by 8, a full 16->16 (1,16) convolution in stage 2 pooled by 2, and Linear(16*T3 -> dim_token) over
 * the flattened map (T3 = 16 for the reference's 250-sample window; isd_cvblock_flat_dim returns 16*T3).
 * Flat parameter block: conv1.weight [8,1,1,64] | bn1.weight [8] | bn1.bias [8] | conv2.weight [16,1,C,1] |
 *   bn2.weight [16] | bn2.bias [16] | conv3.weight [16,16,1,16] | bn3.weight [16] | bn3.bias [16] |
 *   projector.weight [F, 16*T3] | projector.bias [F];  buffer block as above (bn1, bn2, bn3). */
int isd_cvblock_plan_create(isd_eegnet_plan** out, int in_channels, int dim_token, int T);
int64_t isd_cvblock_flat_dim(const isd_eegnet_plan* plan);
/* Optional device-resident dropout step counter (uint64): when set, every pass mixes its current value into the dropout
 * seed, so a captured HIP graph -- which replays the same seed argument -- draws new masks by incrementing the counter
 * inside the graph.  Null (the default) = the seed argument alone. */
int isd_eegnet_plan_set_seed_counter(isd_eegnet_plan* plan, const uint64_t* seed_dev);
/* Element type of the input x of every isd_eegnet_* call on this plan (forward, backward, the _stage forms, zone-batched
 * calls): ISD_ACT_F32 (the default) or ISD_ACT_BF16, x then being [B][C][T] bf16 passed through the same const float*
 * argument (e.g. the map of isd_features_fused_bf16).  bf16 values are widened to fp32 on load, which is exact, and the
 * head then computes exactly what it computes in fp32 on those values: same kernels, same order, the same bits as an
 * fp32 call on the widened input.  It is not autocast: the head's arithmetic stays fp32 throughout.  No input
 * gradient: isd_eegnet_backward_x returns ISD_ERR_UNSUPPORTED on a bf16 plan. */
int isd_eegnet_plan_set_input_dtype(isd_eegnet_plan* plan, int dtype);
int isd_eegnet_plan_destroy(isd_eegnet_plan* plan);
int64_t isd_eegnet_param_count(const isd_eegnet_plan* plan);
int64_t isd_eegnet_buffer_count(const isd_eegnet_plan* plan);
/* exactly what the passes address, every region from a 256-byte line; the linear layer's region is
 * isd_linear_workspace_bytes and 64 floats of slack */
int64_t isd_eegnet_workspace_bytes(const isd_eegnet_plan* plan, int64_t B);
int isd_eegnet_forward(const isd_eegnet_plan* plan, const float* x, const float* params, float* buffers,
                       float* out, void* workspace, int64_t B, int training, float momentum, float eps,
                       float dropout_p, uint64_t seed, void* stream);
int isd_eegnet_backward(const isd_eegnet_plan* plan, const float* x, const float* params, const float* dout,
                        float* dparams, void* workspace, int64_t B, float dropout_p, uint64_t seed,
                        void* stream);
/* The same plus the gradient w.r.t. the input trials, dx [B][C][T] (fast.py:203-210 asks for an autograd-differentiable
 * encoder; the attribution scripts differentiate the network w.r.t. x).  `training` = the value the forward was called
 * with: 1 (batch statistics: BatchNorm's mean / variance paths reach dx) or 2 (isd_eegnet_forward(..., training = 2):
 * eval-mode statistics with the activations kept for this call -- what attribution methods use).  Single device. */
int isd_eegnet_backward_x(const isd_eegnet_plan* plan, const float* x, const float* params, const float* dout,
                          float* dparams, float* dx, void* workspace, int64_t B, int training, float dropout_p,
                          uint64_t seed, void* stream);
/* Synchronised BatchNorm under data parallelism (the reference's heads use plain nn.BatchNorm2d on one
 * device, fast.py:46-63,133-159, so the single-device batch statistics are what a sharded batch must reproduce).
 * The forward and backward passes above are four stages each (0..3); after stages 0, 1 and 2 a block of fp64 batch
 * sums is complete in the workspace (isd_eegnet_sync_block gives its byte offset and length).  The caller runs the
 * stages one by one with the same arguments on every rank, all-reduces (SUM) that block between two stages, and
 * passes the number of ranks (equal shards): the statistics are then those of the global batch, and the parameter
 * gradients sum to the single-device gradient under the usual gradient all-reduce.  world = 1 without all-reduces is
 * isd_eegnet_forward / isd_eegnet_backward.  Evaluation (training == 0) needs no exchange. */
int isd_eegnet_forward_stage(const isd_eegnet_plan* plan, int stage, const float* x, const float* params,
                             float* buffers, float* out, void* workspace, int64_t B, int training, float momentum,
                             float eps, float dropout_p, uint64_t seed, int world, void* stream);
int isd_eegnet_backward_stage(const isd_eegnet_plan* plan, int stage, const float* x, const float* params,
                              const float* dout, float* dparams, void* workspace, int64_t B, float dropout_p,
                              uint64_t seed, int world, void* stream);
int isd_eegnet_sync_block(const isd_eegnet_plan* plan, int64_t B, int backward, int stage, int64_t* byte_offset,
                          int64_t* n_doubles);
/* What the 8-byte words of that block are: 0 = fp64 sums, 1 = the int64 words of exact accumulators (the partial sums of
 * the workgroups are added with integer atomics so that a pass gives the same bits on every run -- the reference's
 * cudnn.deterministic, src/fast/utils.py:104-114); all-reduce the block with that element type (SUM either way). */
int isd_eegnet_sync_block_kind(int backward, int stage);

/* ------------------------------------------------------------------------
 * Transformer tail of FAST (src/fast/models/fast.py:10-29 AttentionBlock, :260-268 forward_transformer).
 * The dense projections are isd_linear_* launches over the [B*S, D] token matrix; these are the pieces around them.
 *   embed:      tok[b,0] = cls + pos[0];  tok[b,1+n] = x[b,n] + pos[1+n]                 (fast.py:263-265)
 *   layernorm:  nn.LayerNorm(D), D <= 64; stats [M][3] = (mean, rstd, mean_lo) saved for backward: the row's mean
 *               is mean + mean_lo, mean_lo the part below fp32's precision of mean              (fast.py:11,13)
 *   attention:  nn.MultiheadAttention core, batch_first: qkv [B][S][3D] (q|k|v) -> ctx [B][S][D], probs [B][H][S][S];
 *               S <= 8 tokens, head_dim <= 8; attention dropout through a counter-based mask (seed)   (fast.py:12,23)
 * ---------------------------------------------------------------------- */
int isd_embed_forward(const float* x, const float* cls, const float* pos, float* tok, int64_t B, int N, int D,
                      void* stream);
int isd_embed_backward(const float* dtok, float* dx, float* dcls, float* dpos, int64_t B, int N, int D,
                       void* stream);
int isd_layernorm_forward(const float* x, const float* w, const float* b, float* y, float* stats, int64_t M, int D,
                          float eps, void* stream);
int isd_layernorm_backward(const float* x, const float* w, const float* dy, const float* stats, float* dx,
                           float* dw, float* db, int64_t M, int D, void* stream);
int isd_attention_forward(const float* qkv, float* ctx, float* probs, int64_t B, int S, int H, int head_dim,
                          float dropout_p, uint64_t seed, void* stream);
int isd_attention_backward(const float* qkv, const float* probs, const float* dctx, float* dqkv, int64_t B, int S,
                           int H, int head_dim, float dropout_p, uint64_t seed, void* stream);

/* ----------------------------------------------------------------------
 * The whole transformer tail in ONE launch per direction (replaces the per-operator sequence above for
 * FAST.forward_transformer, src/fast/models/fast.py:260-268 with AttentionBlock :10-29 -- the mode the reference
 * trains, src/fast/train/trainer.py:58):
 *   tokens = cat(cls, tokin) + pos[:N+1] -> L x [x += MHA(LN1 x); x += drop(W2 drop(gelu(W1 LN2 x)))] ->
 *   logits = last_layer(drop(x[:, 0])).
 * params: ONE flat f32 block,  pos_embedding [n_pos][D] | cls_token [D] | per block: layer_norm_1.{weight,bias} |
 *   attn.in_proj_{weight [3D][D], bias} | attn.out_proj.{weight,bias} | layer_norm_2.{weight,bias} |
 *   linear.0.{weight [2D][D], bias} | linear.3.{weight [D][2D], bias} | last_layer.{weight [n_cls][D], bias}
 *   (isd_tail_fused_param_count floats).  tokin [B][N][D] = input_layer's output; logits [B][n_cls].
 * Training: `save` (isd_tail_fused_save_floats(B, N+1, D, L) floats) and xfinal [B][D] receive what the backward
 *   needs; both null for inference (then every dropout probability must be 0).  Dropout masks are counter-based:
 *   pass the same seed to the backward.  seed_dev (may be null) points at a device-resident step counter that is
 *   mixed into the seed at launch: a captured HIP graph replays the same arguments, and advances its masks by
 *   incrementing that counter inside the graph.
 * Backward: dlogits [B][n_cls] -> dtokin [B][N][D] and dparams (the block's layout, overwritten; positional rows past
 *   N+1 get zeros); workspace = isd_tail_fused_workspace_floats floats (one partial block per wave, summed in a
 *   fixed order: deterministic).
 * Needs dim_token 16 or 32, hidden = 2 dim_token, N + 1 <= 8 tokens, head width 4 or 8, L <= 8, n_cls <= 16
 * (isd_tail_fused_supported; the per-operator entry points cover everything else).
 * ---------------------------------------------------------------------- */
int isd_tail_fused_supported(int N, int D, int H, int L, int hidden, int n_cls);
int64_t isd_tail_fused_param_count(int n_pos, int D, int L, int n_cls);
int64_t isd_tail_fused_save_floats(int64_t B, int S, int D, int L);
int64_t isd_tail_fused_workspace_floats(int64_t B, int N, int n_pos, int D, int L, int n_cls);
int isd_tail_fused_forward(const float* params, const float* tokin, float* logits, float* save, float* xfinal,
                           int64_t B, int N, int n_pos, int D, int H, int L, int hidden, int n_cls, float p_attn,
                           float p_mlp, float p_cls, uint64_t seed, const uint64_t* seed_dev, void* stream);
int isd_tail_fused_backward(const float* params, const float* save, const float* xfinal, const float* dlogits,
                            float* dtokin, float* dparams, float* workspace, int64_t B, int N, int n_pos, int D, int H,
                            int L, int hidden, int n_cls, float p_attn, float p_mlp, float p_cls, uint64_t seed,
                            const uint64_t* seed_dev, void* stream);

/* ----------------------------------------------------------------------
 * Whole classifier step on spec-S features in one call (the build-defined classifier of SURVEY 8d:
 * Conv4Layers(nb*C, 32) -> Linear(32, n_cls) -> softmax cross-entropy; replaces the call sequence
 * isd_conv4_forward / isd_linear_forward / isd_softmax_ce / isd_linear_backward / isd_conv4_backward).
 *   x [B][c_total][T] f32 features, params = the conv4 flat block, fc_w [n_cls][32], fc_b [n_cls].
 *   labels (uint8 / int64, may be null: inference): loss = sum_b nll_b * grad_scale, gradients scaled alike.
 *   dparams (conv4 layout) and dfc ([n_cls][32] then [n_cls]) may be null: forward + loss only.
 * Needs one zone, 4 layers, 32 filters, fp32 activations, T - 4 <= 16 output steps, n_cls <= 16
 * (isd_featcnn_supported); workspace = isd_conv4_workspace_bytes(plan, B, T).
 * ---------------------------------------------------------------------- */
int isd_featcnn_supported(const isd_conv4_plan* plan, int64_t B, int64_t T, int n_cls);
/* Which kernels the calling thread's last first-layer forward and weight gradient launched (isd_conv4_forward /
 * _backward on the layerwise route, isd_featcnn_step): forward + 16 * weight gradient.  Forward: 0 the general
 * kernel, 1..4 the LDS-DMA kernel for wide inputs as <filter tiles, column tiles per wave> = <2, 2>, <2, 4>, <1, 2>,
 * <1, 4>, 5 the bf16 matrix-core kernel.  On the fused routes isd_conv4_forward runs the whole stack in one kernel
 * and reports that instead: 6 the fused fp32 forward, 7 the fused bf16 forward (the fused backward kernels leave the
 * weight-gradient code as it was).  Weight gradient: 0 general, 1 wide fp32, 2 wide bf16.  For tests: a fall-back to
 * another kernel must not pass for the intended one. */
int isd_first_layer_last_path(void);
/* The stage loop of the calling thread's last wide fp32 weight gradient (code 1 above): 0 the generic loop, 1 the
 * instance that runs full stages of four 13-step items as straight-line code.  Both compute the same bits. */
int isd_first_wgrad_last_stage_loop(void);
int isd_featcnn_step(const isd_conv4_plan* plan, const float* x, const float* params, const float* fc_w,
                     const float* fc_b, const void* labels, int label_bytes, float* dparams, float* dfc,
                     float* logits, int64_t* pred, float* loss, void* workspace, int64_t B, int64_t T, int n_cls,
                     float grad_scale, void* stream);
/* BASELINE config 3 with the feature map itself in bf16: x [B][c_total][T] bf16 as written by
 * isd_features_fused_bf16 (the first layer rounds an fp32 map to bf16 as it packs its operands: the results are bit
 * for bit those of isd_featcnn_step on the same values).  The plan must have bf16 activations and a multiple of 8
 * input channels; ISD_ERR_UNSUPPORTED otherwise. */
int isd_featcnn_step_bf16(const isd_conv4_plan* plan, const uint16_t* x, const float* params, const float* fc_w,
                          const float* fc_b, const void* labels, int label_bytes, float* dparams, float* dfc,
                          float* logits, int64_t* pred, float* loss, void* workspace, int64_t B, int64_t T,
                          int n_cls, float grad_scale, void* stream);

/* One AdamW step on a flat fp32 block (replaces the optimizer of the reference's training loop,
 * src/fast/train/trainer.py:49 `optim.AdamW(self.parameters(), lr=0.0005)`: decoupled weight decay, torch's
 * operation order -- p *= 1 - lr wd; m += (g - m)(1 - b1); v = b2 v + (1 - b2) g g;
 * p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)).  params / grads / exp_avg / exp_avg_sq: n floats each,
 * 16-byte aligned, device memory; exp_avg and exp_avg_sq start at zero.  `step` = t >= 1 of THIS step.  lr_dev /
 * step_dev (optional, device memory): learning rate and step count read by the kernel instead of the by-value
 * arguments, so that a captured HIP graph can replay the step (the caller advances *step_dev before each replay). */
int isd_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int64_t step, const float* lr_dev,
                   const int64_t* step_dev, void* stream);
/* The same update over a list of tensors in one launch (per 96 tensors): host arrays of n_tensors DEVICE pointers and
 * element counts; tensors need not be aligned or adjacent.  step_dev (optional): FOUR int64 in device memory, zero
 * before the first step -- [0] = steps taken so far: the kernel uses t = [0] + 1 and stores it back itself; [1] is its
 * scratch; [2], [3] hold beta1^t, beta2^t as doubles (kept by recurrence; to resume at step t > 0 store the bit
 * patterns of beta^t there) -- so a captured graph replays the step with nothing to advance on the host. */
int isd_adamw_multi_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2,
                         double eps, double weight_decay, int64_t step, const float* lr_dev, int64_t* step_dev,
                         void* stream);

/* ----------------------------------------------------------------------
 * HeadConv_Paper_Version  (replaces src/fast/models/fast.py:170-196 behind the head contract :203-210)
 *   x [B][C][T] f32 -> out [B][feature_dim];  feature_dim in [3,64] (F1 = F/2, F2 = F3 = F/3, F4 = F), T >= 46.
 * Flat parameter block (reference state_dict order, trainable tensors only):
 *   cnn1_t.weight [F1,1,1,3] | cnn1_t.bias [F1] | cnn1_s.weight [F1,F1,C,1] | norm1.weight [F1] | norm1.bias [F1] |
 *   cnn2.weight [F2,F1,1,3] | norm2.weight | norm2.bias | cnn3.weight [F3,F2,1,3] | norm3.* | cnn4.weight [F4,F3,1,3] |
 *   norm4.weight | norm4.bias
 * Buffer block: running_mean / running_var of norm1..norm4 (F1,F1,F2,F2,F3,F3,F4,F4 floats), updated when training.
 * training != 0: batch statistics (biased variance to normalise, unbiased for the running update).  MaxPool ties
 * route the gradient to the first element, as torch does.  backward: parameter gradients only (x is data); one
 * backward per train-mode forward, same workspace.
 * ---------------------------------------------------------------------- */
typedef struct isd_paperhead_plan isd_paperhead_plan;
int isd_paperhead_plan_create(isd_paperhead_plan** out, int in_channels, int feature_dim, int T);
int isd_paperhead_plan_destroy(isd_paperhead_plan* plan);
int64_t isd_paperhead_param_count(const isd_paperhead_plan* plan);
int64_t isd_paperhead_buffer_count(const isd_paperhead_plan* plan);
int64_t isd_paperhead_workspace_bytes(const isd_paperhead_plan* plan, int64_t B);   /* exactly what the passes address */
int isd_paperhead_forward(const isd_paperhead_plan* plan, const float* x, const float* params, float* buffers,
                          float* out, void* workspace, int64_t B, int training, float momentum, float eps, void* stream);
int isd_paperhead_backward(const isd_paperhead_plan* plan, const float* x, const float* params, const float* dout,
                           float* dparams, void* workspace, int64_t B, void* stream);
/* ... plus the gradient w.r.t. the input trials dx [B][C][T]; training = 1 after a batch-statistics forward, 0 after an
 * eval-mode forward (running statistics). */
int isd_paperhead_backward_x(const isd_paperhead_plan* plan, const float* x, const float* params, const float* dout,
                             float* dparams, float* dx, void* workspace, int64_t B, int training, void* stream);
/* Synchronised BatchNorm under data parallelism, as for the EEGNet head: forward stages 0..4 and backward stages 0..4;
 * after stage s < 4 one layer's block of fp64 batch sums (isd_paperhead_sync_block) is complete in the workspace and
 * the caller all-reduces it (SUM) before the next stage; `world` scales the counts and pre-divides the gamma / beta
 * gradients, which every rank assembles from global sums. */
int isd_paperhead_forward_stage(const isd_paperhead_plan* plan, int stage, const float* x, const float* params,
                                float* buffers, float* out, void* workspace, int64_t B, int training, float momentum,
                                float eps, int world, void* stream);
int isd_paperhead_backward_stage(const isd_paperhead_plan* plan, int stage, const float* x, const float* params,
                                 const float* dout, float* dparams, void* workspace, int64_t B, int world, void* stream);
int isd_paperhead_sync_block(const isd_paperhead_plan* plan, int64_t B, int backward, int stage, int64_t* byte_offset,
                             int64_t* n_doubles);
int isd_paperhead_sync_block_kind(int backward, int stage);   /* as isd_eegnet_sync_block_kind */

/* ------------------------------------------------------------------------
 * Zone-batched launches for the one-encoder-per-zone heads (Head.encoders, fast.py:203-210: eight EEGNet_Encoder /
 * CVBlock / HeadConv_Paper_Version instances on eight channel subsets).  Between isd_zone_batch_begin() and
 * isd_zone_batch_launch() the calls
 *   isd_eegnet_forward / isd_eegnet_backward / isd_paperhead_forward / isd_paperhead_backward
 * made by THIS thread record their kernel launches instead of issuing them; isd_zone_batch_next() separates the
 * zones (at most 8).  isd_zone_batch_launch() then issues launch i of all zones as ONE kernel (blockIdx.z = zone).
 * The zones must make the same calls on plans of the same kind, batch and length (channel counts may differ); a
 * call that cannot be recorded fails and poisons the batch (isd_zone_batch_launch then returns ISD_ERR_INVALID).
 * Nothing is read on the host in between: the recorded calls only have to use the stream given to the launch. */
int isd_zone_batch_begin(void);
int isd_zone_batch_next(void);
int isd_zone_batch_launch(void* stream);
int isd_zone_batch_abort(void);

/* ----------------------------------------------------------------------
 * TSception, the deep comparison model (replaces the TSception class of scripts/train_tsception.py:39-119):
 *   x [B][C][T] f32 -> three temporal filter banks (k1, k2, k3 taps; Conv2d(1, num_T, (1, k)) + bias + LeakyReLU(0.01)
 *   + AvgPool(8), concatenated along time) -> BN_t -> Sception1 (all C rows) and Sception2 (two blocks of C / 2 rows) +
 *   LeakyReLU + AvgPool(2) -> BN_s -> 3-row fusion conv + LeakyReLU + AvgPool(4) -> BN_fusion -> time mean ->
 *   Linear(num_S, hidden) + ReLU + Dropout + Linear(hidden, n_classes) -> logits [B][n_classes].
 * Flat parameter block (named_parameters() order):
 *   Tception1.0.weight [num_T,1,1,k1] | Tception1.0.bias [num_T] | Tception2.0.* (k2) | Tception3.0.* (k3) |
 *   Sception1.0.weight [num_S,num_T,C,1] | .bias [num_S] | Sception2.0.weight [num_S,num_T,C/2,1] | .bias |
 *   fusion_layer.0.weight [num_S,num_S,3,1] | .bias | BN_t.weight | BN_t.bias [num_T] | BN_s.weight | BN_s.bias |
 *   BN_fusion.weight | BN_fusion.bias [num_S] | fc.0.weight [hidden,num_S] | fc.0.bias | fc.3.weight
 *   [n_classes,hidden] | fc.3.bias
 * Buffer block: running_mean / running_var of BN_t, BN_s, BN_fusion (num_T, num_T, num_S, num_S, num_S, num_S floats),
 *   updated when training (biased variance normalises, unbiased feeds running_var).
 * Envelope: 2 <= C <= 128, C != 3; 1 <= taps <= 512; T with at least 8 valid samples at every tap count and at least
 *   one sample after the fusion pool; num_T, num_S <= 16; hidden <= 64; n_classes <= 16.  Anything else:
 *   ISD_ERR_INVALID from plan_create with the reason in isd_last_error().
 * B <= 350 trials per pass (the largest batch the kernels have been run and checked at; workspace_bytes, forward and
 *   backward return ISD_ERR_INVALID above it: split a larger batch).
 * Dropout is counter-based on (seed, trial, unit): pass the same seed and probability to the backward.  backward:
 *   parameter gradients only (dparams in the block's layout, overwritten), after a forward on the same workspace --
 *   batch statistics after training != 0, running statistics otherwise.  No un-pooled temporal map is written in
 *   either direction; every batch sum is exact or added in a fixed order: a step is bitwise repeatable.
 * ---------------------------------------------------------------------- */
typedef struct isd_tsception_plan isd_tsception_plan;
int isd_tsception_plan_create(isd_tsception_plan** out, int in_channels, int T, int k1, int k2, int k3, int num_T,
                              int num_S, int hidden, int n_classes);
int isd_tsception_plan_destroy(isd_tsception_plan* plan);
int64_t isd_tsception_param_count(const isd_tsception_plan* plan);
int64_t isd_tsception_buffer_count(const isd_tsception_plan* plan);
/* exactly what the passes address, in whole 256-byte lines */
int64_t isd_tsception_workspace_bytes(const isd_tsception_plan* plan, int64_t B);
int isd_tsception_forward(const isd_tsception_plan* plan, const float* x, const float* params, float* buffers,
                          float* logits, void* workspace, int64_t B, int training, float momentum, float eps,
                          float dropout_p, uint64_t seed, void* stream);
int isd_tsception_backward(const isd_tsception_plan* plan, const float* x, const float* params, const float* dlogits,
                           float* dparams, void* workspace, int64_t B, float dropout_p, uint64_t seed, void* stream);
/* Measurement only (tools/bench_tsception.py): the temporal stage's kernels alone on a workspace that a forward and a
 * backward of the same B have been run on (what they left there is read as the pooled map, its gradient and BN_t's
 * backward coefficients; any finished pass will do for timing, the values are not meaningful) -- backward == 0 the
 * fused filter + LeakyReLU + pool pass, else the three weight-gradient kernels (their partial sums are left in the
 * workspace, not reduced).  Same refusals as forward (batch bound, an open zone batch). */
int isd_tsception_temporal_probe(const isd_tsception_plan* plan, const float* x, const float* params, void* workspace,
                                 int64_t B, int backward, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISD_HIP_H */
