/*
 * dsptoolbox_amd -- C-ABI of the MI355X (gfx950) spectral hot path.
 *
 * The reference (dsptoolbox 0.8) is pure Python and has no FFI; its "plugin
 * boundary" for this path is the ndarray-in / ndarray-out private backend layer
 * (SURVEY.md section 1, L2).  Each entry point below replaces one of those backend
 * functions; the Python host shim (dsptoolbox_amd/backend.py) binds them with
 * ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; the message is
 *     available through ds_last_error().  Nothing throws across the ABI.
 *   - signals are PLANAR fp32: channel c, sample n at x[c*ld + n]
 *     (the reference stores (samples, channels) float64; the shim transposes).
 *   - outputs are written in the reference's axis order so the host only
 *     casts: (bins, channels), (bins, frames, channels), (bins, ch, ch).
 *   - `_dev` variants take DEVICE pointers (inputs already resident in HBM,
 *     nothing is copied, everything is enqueued on the context's stream and
 *     NOT synchronised).  The plain variants take HOST pointers, stage through
 *     the context's workspace and return after the result is in host memory.
 *   - a ds_ctx is bound to one device and one HIP stream; not re-entrant.
 */
#ifndef DSPTOOLBOX_AMD_H
#define DSPTOOLBOX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ds_ctx ds_ctx;
typedef struct { float re, im; } ds_c32;

/* error codes */
#define DS_OK            0
#define DS_ERR_ARG      -1   /* invalid argument (shape, size, null pointer)   */
#define DS_ERR_UNSUP    -2   /* valid in the reference, not built yet on GPU   */
#define DS_ERR_HIP      -3   /* HIP runtime error                              */
#define DS_ERR_NOMEM    -4
#define DS_ERR_COMM     -5   /* RCCL error                                     */

/* transfer-function modes: transfer_functions/enums.py:4-16 */
#define DS_TF_H1 1
#define DS_TF_H2 2
#define DS_TF_H3 3

/* Welch averaging over frames: _spectral_methods.py:151-162 */
#define DS_AVG_MEAN   0
#define DS_AVG_MEDIAN 1

/* filter-bank modes: standard/enums.py:279-292 */
#define DS_FB_PARALLEL   1
#define DS_FB_SEQUENTIAL 2
#define DS_FB_SUMMED     3

/* ---- context, memory, timing ------------------------------------------- */
int         ds_version(void);
int         ds_device_count(void);
int         ds_init(int device, ds_ctx** out);
void        ds_destroy(ds_ctx* ctx);
const char* ds_last_error(ds_ctx* ctx);            /* ctx may be NULL          */
int         ds_malloc(ds_ctx* ctx, void** dptr, size_t bytes);
int         ds_free(ds_ctx* ctx, void* dptr);
/* Page-locked host memory for result staging (device-resident signals): a download into
 * it runs at the link's rate and needs no driver-side bounce buffer.  Plumbing: nothing in the reference.     */
int         ds_host_alloc(ds_ctx* ctx, void** hptr, size_t bytes);
int         ds_host_free(ds_ctx* ctx, void* hptr);
int         ds_upload(ds_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int         ds_download(ds_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int         ds_memset(ds_ctx* ctx, void* dst_dev, int value, size_t bytes);
int         ds_sync(ds_ctx* ctx);
/* hipEvent pair recorded on the context's stream (bench.py's live kernel time) */
int         ds_timer_start(ds_ctx* ctx);
int         ds_timer_stop(ds_ctx* ctx, float* elapsed_ms);
/* per-kernel HIP-event timing on the context's stream: while enabled every
 * kernel launch is bracketed by an event pair; ds_profile_report synchronises
 * and returns "name total_ms launches\n" lines for the launches since the
 * previous report (string owned by the context).                             */
int         ds_profile_enable(ds_ctx* ctx, int on);
const char* ds_profile_report(ds_ctx* ctx);
/* restrict the bracketing to one kernel name (NULL or "": all kernels): every
 * event pair costs ~3 us of stream time, which matters for 10 us kernels      */
int         ds_profile_only(ds_ctx* ctx, const char* kernel_name);
/* bracket only every `every`-th matching launch (1 = all): an event pair costs ~3 us of stream time */
int         ds_profile_stride(ds_ctx* ctx, int every);
/* what an event pair adds to the kernels it brackets: n_kernels empty kernels bracketed the same
 * way, average over reps, in ms.  b1 (one kernel) and b2 (two) give 2 b1 - b2, a lower bound of the
 * bracket's fixed cost (bench.py reports kernel times with and without it) */
int         ds_profile_overhead(ds_ctx* ctx, int reps, int n_kernels, double* ms);
/* which kernel family ran: the launch names since the previous call, space separated, each "group" or
 * "group@variant" (e.g. "csm_gemm@b3", "fir@4k_p2"; string owned by the context).  The library reads its
 * DSPTOOLBOX_AMD_* switches once, in ds_init (csrc/config.hpp); tests open a context under a switch and
 * check here that the other family really computed the result.                                          */
const char* ds_routes(ds_ctx* ctx);
/* max FFT length one workgroup transforms inside LDS (complex points)       */
int         ds_max_fft_len(void);

/* ---- STFT: replaces _stft, standard/_spectral_methods.py:176-282 --------
 * frame k of channel c = samples [k*hop - pad_front, k*hop - pad_front + W)
 * (out-of-range samples read as 0, which is the reference's zero padding:
 * helpers/other.py:181-213), times window[W]; optional detrend (mean of the
 * windowed frame, :264-265); rFFT of length nfft (crop / zero-pad, :268);
 * out[b][k][c] *= scale, bins 0 and nfft/2 additionally *= edge_scale;
 * power != 0 stores |.|^2 in .re (:271-278).  B = nfft/2 + 1.               */
int ds_stft_r2c_dev(ds_ctx* ctx, const float* x_dev, int64_t n_samples, int n_ch,
                    int64_t ld, int W, int hop, int nfft, int64_t pad_front,
                    int n_frames, const float* window_dev, int detrend,
                    float scale, float edge_scale, int power, ds_c32* out_dev);
int ds_stft_r2c(ds_ctx* ctx, const float* x, int64_t n_samples, int n_ch,
                int W, int hop, int nfft, int64_t pad_front, int n_frames,
                const float* window, int detrend, float scale, float edge_scale,
                int power, ds_c32* out);

/* ---- Welch spectra: replaces _welch, _spectral_methods.py:10-173 ---------
 * Raw frame averages Sxx=mean|X|^2, Syy=mean|Y|^2, Sxy=mean conj(X)Y over
 * n_frames frames (frame k = samples [k*hop, k*hop+W), zero padded), then the
 * reference's finish(): S *= norm_scale (1, 1/W^2, 1/W for the three FFT
 * norms, enums.py:53-75); if halve_edges: S *= factor and bins 0, W/2 halved
 * (:165-168); if amp_sqrt: principal sqrt (:170-171).  average = DS_AVG_MEDIAN takes the
 * per-bin median over frames (real and imaginary parts separately) times the
 * reference's bias n (:153-162) instead of the mean.
 *
 * ds_welch_tf: replaces compute_transfer_function,
 * transfer_functions/transfer_functions.py:419-539.  n_cx is 1 (one input for
 * every output channel) or n_cy (pairwise).  tf[b][c] (B x n_cy), coh[b][c].
 *
 * ds_welch_psd: auto spectra of every channel of x (psd[b][c], B x n_cx) --
 * Signal.get_spectrum with the Welch method, classes/signal.py:881-897.      */
int ds_welch_tf_dev(ds_ctx* ctx, const float* x_dev, int n_cx, int64_t ldx,
                    const float* y_dev, int n_cy, int64_t ldy, int64_t n_samples,
                    int W, int hop, int n_frames, const float* window_dev,
                    int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                    double factor, int halve_edges, ds_c32* tf_dev, float* coh_dev);
int ds_welch_tf(ds_ctx* ctx, const float* x, int n_cx, const float* y, int n_cy,
                int64_t n_samples, int W, int hop, int n_frames, const float* window,
                int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                double factor, int halve_edges, ds_c32* tf, float* coh);
/* the same with the reference's array layout at the boundary: x (n_samples, n_cx), y (n_samples,
 * n_cy) float64 C-order (classes/signal.py:222-301).  The cast + transpose to planar float32 runs
 * on host threads straight into pinned chunks whose DMA overlaps the next chunk's cast.        */
/* float64 on both sides (the copy back runs through the same pinned chunks, widened / interleaved by
 * host threads while the next chunk's DMA is in flight): STFT (bins, frames, channels) complex128
 * as interleaved doubles; FIR y (bands or 1, n_samples, n_ch) float64.                            */
int ds_stft_r2c_f64(ds_ctx* ctx, const double* x, int64_t n_samples, int n_ch, int W, int hop,
                    int nfft, int64_t pad_front, int n_frames, const float* window, int detrend,
                    float scale, float edge_scale, int power, double* out_c128);
/* the same for whole-signal spectra, one-item spectral division and the inverse STFT (round 4): float64 /
 * complex128 arrays in the reference's own layouts on both sides, cast in host threads through pinned chunks
 * while the previous chunk's copy is in flight.  spec (bins, channels) complex128; ir (n_out, channels) float64;
 * stft (bins, frames, channels) complex128 in, out (total_length, channels) float64.                          */
int ds_rfft_f64(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, int n_fft, float scale,
                double* spec_c128);
int ds_deconv_f64(ds_ctx* ctx, const double* y, int n_ch, int64_t n_samples, int n_fft, const ds_c32* r,
                  int r_per_channel, int64_t n_out, double* ir);
int ds_istft_f64(ds_ctx* ctx, const double* stft_c128, int n_bins, int n_frames, int n_ch, int nfft, int W,
                 int step, int frame_offset, int n_frames_total, const float* window, float scale,
                 int64_t total_length, double* out);
int ds_fir_ola_f64(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, const float* taps,
                   int n_filt, int n_taps, int mode, double* y);
int ds_welch_psd_f64(ds_ctx* ctx, const double* x, int n_cx, int64_t n_samples, int W, int hop,
                     int n_frames, const float* window, int detrend, int average, int amp_sqrt,
                     double norm_scale, double factor, int halve_edges, float* psd);
int ds_csm_f64(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, int W, int hop,
               int n_frames, const float* window, int detrend, int average, int amp_sqrt,
               double norm_scale, double factor, int halve_edges, ds_c32* csm);
int ds_welch_tf_f64(ds_ctx* ctx, const double* x, int n_cx, const double* y, int n_cy,
                    int64_t n_samples, int W, int hop, int n_frames, const float* window,
                    int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                    double factor, int halve_edges, ds_c32* tf, float* coh);
/* The same estimate in float64 END TO END (transforms, sums, finish) for small or ill-conditioned
 * problems: x (n_samples, n_cx), y (n_samples, n_cy) float64 C-order exactly as the reference
 * holds them, float64 window, mean or median averaging (median: at most 4096 frames), W a power
 * of two <= 262144 (16384: as the 8192-point complex transform of the even / odd samples; 2^15 ... 2^18: one
 * decimation-in-frequency stage in front of that transform); tf[b][c] complex128
 * (interleaved re, im), coh[b][c] float64.  With fp32 transforms every frame's rounding floor
 * (1e-7 of its peak) lands on all bins, so bins 80 dB down -- the top of a fast pink sweep,
 * BASELINE config 1 -- are only good to 1e-4; this route keeps the reference's 1e-12.        */
int ds_welch_tf_x64(ds_ctx* ctx, const double* x, int n_cx, const double* y, int n_cy,
                    int64_t n_samples, int W, int hop, int n_frames, const double* window,
                    int detrend, int average, int mode, int amp_sqrt, double norm_scale,
                    double factor, int halve_edges, double* tf, double* coh);
/* _welch itself in float64 end to end (_spectral_methods.py:10-173): auto spectra (y NULL) or the cross
 * spectra conj(X_i) Y_i of channel pairs, mean or median averaging; x, y (n_samples, n_ch) float64 C order,
 * out [nb][n_ch] complex128 (auto spectra: imaginary part 0).  What the host mirror takes for SHORT
 * estimates (fewer than 128 frames: no averaging-down of the fp32 transform rounding).                     */
int ds_welch_spec_x64(ds_ctx* ctx, const double* x, const double* y, int n_ch, int64_t n_samples, int W,
                      int hop, int n_frames, const double* window, int detrend, int average, int amp_sqrt,
                      double norm_scale, double factor, int halve_edges, double* out);
/* _csm_welch in float64 end to end (_spectral_methods.py:285-371; up to 1024 channels; average = median, the
 * per-pair median of _welch :153-162, up to 128 frames): csm [nb][n_ch][n_ch] complex128, same element order as ds_csm. */
int ds_csm_x64(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, int W, int hop, int n_frames,
               const double* window, int detrend, int average, int amp_sqrt, double norm_scale, double factor,
               int halve_edges, double* csm);
int ds_welch_psd_dev(ds_ctx* ctx, const float* x_dev, int n_cx, int64_t ldx,
                     int64_t n_samples, int W, int hop, int n_frames,
                     const float* window_dev, int detrend, int average, int amp_sqrt,
                     double norm_scale, double factor, int halve_edges, float* psd_dev);
int ds_welch_psd(ds_ctx* ctx, const float* x, int n_cx, int64_t n_samples, int W,
                 int hop, int n_frames, const float* window, int detrend, int average,
                 int amp_sqrt, double norm_scale, double factor, int halve_edges,
                 float* psd);
/* cross spectrum of channel pairs (x[c], y[c]) -- _welch(x, y): csd[b][c]     */
int ds_welch_csd(ds_ctx* ctx, const float* x, const float* y, int n_ch,
                 int64_t n_samples, int W, int hop, int n_frames, const float* window,
                 int detrend, int average, int amp_sqrt, double norm_scale, double factor,
                 int halve_edges, ds_c32* csd);
/* ... taking the reference's (n_samples, n_ch) float64 C-order arrays as they are (cast + transpose in host threads
 * straight into page-locked upload chunks, like ds_welch_psd_f64 / ds_welch_tf_f64)                                  */
int ds_welch_csd_f64(ds_ctx* ctx, const double* x, const double* y, int n_ch,
                     int64_t n_samples, int W, int hop, int n_frames, const float* window,
                     int detrend, int average, int amp_sqrt, double norm_scale, double factor,
                     int halve_edges, ds_c32* csd);

/* ---- band powers of a spectrogram: replaces np.tensordot(mel_filters, |stft|^2) + to_db in
 * log_mel_spectrogram / mfcc, transforms/transforms.py:181-184, 421-429.
 * stft[b][fc] (n_bins x n_fc, n_fc = frames * channels, the layout ds_stft_r2c writes),
 * weights[band][b]; only bins band_start[band] <= b < band_stop[band] are read (the
 * filters are banded).  out[band][fc] = sum_b w |X|^2, then 10 log10(max(., DBL_MIN)) if
 * to_db, then |DCT-II along the band axis| with NaN -> 0 if dct_abs (MFCC).          */
int ds_band_power_dev(ds_ctx* ctx, const ds_c32* stft_dev, int n_bins, int64_t n_fc,
                      const float* weights_dev, const int* band_start_dev,
                      const int* band_stop_dev, int n_bands, int to_db, int dct_abs,
                      float* out_dev);
int ds_band_power(ds_ctx* ctx, const ds_c32* stft, int n_bins, int64_t n_fc, const float* weights,
                  const int* band_start, const int* band_stop, int n_bands, int to_db,
                  int dct_abs, float* out);

/* ---- delay-and-sum beamformer map on the CSM: replaces the grid x bin loop of
 * BeamformerDASFrequency.get_beamformer_map, beamforming/beamforming.py:853-858:
 * map[g][f] = Re( h_f[:, g]^H  CSM_f  h_f[:, g] ); csm[f][i][j] (n_bins x n_ch x n_ch, the
 * selected bins, diagonal already treated by the caller), h[f][c][g] (the steering
 * vectors, n_bins x n_ch x n_grid), map[g][f].  fp32 MFMA.                        */
int ds_das_map_dev(ds_ctx* ctx, const ds_c32* csm_dev, const ds_c32* h_dev, int n_bins, int n_ch,
                   int n_grid, float* map_dev);
int ds_das_map(ds_ctx* ctx, const ds_c32* csm, const ds_c32* h, int n_bins, int n_ch, int n_grid,
               float* map);
/* The diagonal treatment in front of the map, on the device (beamforming.py:840-845:
 * `csm *= C / (C - 1)` then `np.fill_diagonal(csm[i], 0)` for every bin): out = scale * csm, the
 * diagonal zeroed when zero_diagonal != 0.  csm_dev / out_dev [n_bins][n_ch][n_ch]; out_dev may be
 * csm_dev.  Lets a CSM that ds_csm_dev left in HBM feed ds_das_map_dev without a host round trip.  */
int ds_csm_das_prepare_dev(ds_ctx* ctx, const ds_c32* csm_dev, int n_bins, int n_ch, double scale,
                           int zero_diagonal, ds_c32* out_dev);

/* ---- MVDR, Functional, Orthogonal and CLEAN-SC beamformer maps on the CSM, float64 throughout:
 * replace the per-bin / per-grid-point loops of BeamformerMVDR (beamforming/beamforming.py:1276-1304),
 * BeamformerFunctional (:1177-1210), BeamformerOrthogonal (:1079-1114) and BeamformerCleanSC (:959-997
 * with _clean_sc_deconvolve, beamforming/_beamforming.py:194-297).  csm [f][i][j] complex128 (the
 * selected bins, n_ch x n_ch each), h [f][c][g] complex128 (the steering vectors), map [g][f] float64
 * (before the Simpson integration over f).  n_ch <= 64: one bin's matrix is held in LDS; larger
 * arrays return DS_ERR_UNSUP.
 * ds_bf_eigh: Hermitian eigendecomposition of every bin's matrix (its lower triangle, as numpy's eigh):
 * w [f][k] ascending, v [f][i][k] (column k = eigenvector of w[f][k]).  Complex Jacobi.
 * ds_bf_eig_map: method 0 MVDR map = 1 / sum_k |v_k^H h|^2 / w_k (gamma, n_eig ignored);
 * method 1 Functional map = (q / n)^gamma n with q = sum_k |v_k^H h|^2 sign(w_k)|w_k|^(1/gamma),
 * n = h^H h; method 2 Orthogonal: for e = 0 .. n_eig - 1 (largest eigenvalue first) the grid point i
 * that maximises |v^H h|^2 gets map[i] = |v^H h_i|^2 w (later picks overwrite), every other point 0.
 * ds_bf_cleansc: the CLEAN-SC clean map, at most max_iter iterations of loop gain safety in (0, 1],
 * remove_diagonal != 0 zeroes the CSM's and every source's diagonal.                              */
int ds_bf_eigh_dev(ds_ctx* ctx, const double* a_dev, int n_bins, int n_ch, double* w_dev, double* v_dev);
int ds_bf_eigh(ds_ctx* ctx, const double* a, int n_bins, int n_ch, double* w, double* v);
int ds_bf_eig_map_dev(ds_ctx* ctx, const double* csm_dev, const double* h_dev, int n_bins, int n_ch,
                      int n_grid, int method, double gamma, int n_eig, double* map_dev);
int ds_bf_eig_map(ds_ctx* ctx, const double* csm, const double* h, int n_bins, int n_ch, int n_grid,
                  int method, double gamma, int n_eig, double* map);
int ds_bf_cleansc_dev(ds_ctx* ctx, const double* csm_dev, const double* h_dev, int n_bins, int n_ch,
                      int n_grid, int max_iter, double safety, int remove_diagonal, double* map_dev);
int ds_bf_cleansc(ds_ctx* ctx, const double* csm, const double* h, int n_bins, int n_ch, int n_grid,
                  int max_iter, double safety, int remove_diagonal, double* map);

/* ---- inverse STFT: replaces transforms.istft, transforms/transforms.py:444-586
 * (np.fft.irfft of every frame + _reconstruct_framed_signal,
 * standard/_framed_signal_representation.py:70-137: windowed overlap-add divided by
 * the squared-window envelope clipped at 1e-4).
 * stft[b][f][c] (n_bins x n_frames x n_ch, the layout ds_stft_r2c writes); frames are
 * inverse transformed with length nfft (bins beyond nfft/2 dropped, missing ones zero),
 * scaled by `scale` (the irfft normalisation divided by the physical-unit factor),
 * cropped to W samples and windowed; frame f sits at sample (f + frame_offset)*step of
 * an output of total_length samples whose envelope counts n_frames_total window
 * positions (the reference adds an empty frame before and after unpadded data:
 * frame_offset 1, n_frames_total n_frames + 2).  out[c][n], planar.             */
int ds_istft_dev(ds_ctx* ctx, const ds_c32* stft_dev, int n_bins, int n_frames, int n_ch,
                 int nfft, int W, int step, int frame_offset, int n_frames_total,
                 const float* window_dev, float scale, int64_t total_length,
                 float* out_dev, int64_t ld_out);
int ds_istft(ds_ctx* ctx, const ds_c32* stft, int n_bins, int n_frames, int n_ch, int nfft,
             int W, int step, int frame_offset, int n_frames_total, const float* window,
             float scale, int64_t total_length, float* out);

/* ---- cross-spectral matrix: replaces _csm_welch, _spectral_methods.py:285-371
 * csm[b][i][j], B x C x C; lower triangle csm[b][i2][i1] (i2>=i1) =
 * finish(mean or median over frames of conj(X_i1) X_i2), upper = its conjugate
 * (:351-369).  average: DS_AVG_MEAN (MFMA rank-F update) / DS_AVG_MEDIAN.      */
int ds_csm_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ld, int64_t n_samples,
               int W, int hop, int n_frames, const float* window_dev, int detrend,
               int average, int amp_sqrt, double norm_scale, double factor,
               int halve_edges, ds_c32* csm_dev);
int ds_csm(ds_ctx* ctx, const float* x, int n_ch, int64_t n_samples, int W, int hop,
           int n_frames, const float* window, int detrend, int average, int amp_sqrt,
           double norm_scale, double factor, int halve_edges, ds_c32* csm);
/* bins [bin_start, bin_start + bin_count) only (csm_dev[0] is the matrix of bin_start, mean
 * averaging): the multi-GPU split of the CSM -- every rank transforms all channels and keeps
 * its own bin range, no reduction between ranks.                                         */
int ds_csm_bins_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ld, int64_t n_samples,
                    int W, int hop, int n_frames, const float* window_dev, int detrend,
                    int amp_sqrt, double norm_scale, double factor, int halve_edges,
                    int bin_start, int bin_count, ds_c32* csm_dev);

/* CSM from spectra that are already on hand: X[b][f][c] (n_bins x n_frames x n_ch, the
 * STFT layout) -> csm[b][i][j] = finish(norm_scale/n_frames * sum_f X_i conj X_j).
 * n_frames = 1 replaces _csm_fft, _spectral_methods.py:374-443 (outer product of one
 * whole-signal spectrum; FFTBackward: no finish, others: edges halved, factor, sqrt).     */
int ds_csm_spec_dev(ds_ctx* ctx, const ds_c32* X_dev, int n_bins, int n_frames, int n_ch,
                    int amp_sqrt, double norm_scale, double factor, int halve_edges,
                    ds_c32* csm_dev);
int ds_csm_spec(ds_ctx* ctx, const ds_c32* X, int n_bins, int n_frames, int n_ch, int amp_sqrt,
                double norm_scale, double factor, int halve_edges, ds_c32* csm);

/* ---- whole-signal rFFT / regularised spectral division -------------------
 * ds_rfft: Signal.get_spectrum with SpectrumMethod.FFT, classes/signal.py:899-911
 * (any n_fft >= 2: one-workgroup LDS FFT up to ds_max_fft_len(), four-step FFT for powers
 * of two up to 2^24, Bluestein for every other length up to 2^23; input zero padded).
 * spec[b][c], (n_fft/2+1) x n_ch, multiplied by scale.
 *
 * ds_deconv: replaces _spectral_deconvolve,
 * transfer_functions/_transfer_functions.py:19-42, for a batch of n_items
 * signals of n_ch channels each (planar: y[(item*n_ch + c)*ld + n]).
 * r[(B) or (n_ch x B)] is the regularised inverse conj(X)/(|X|^2+eps) (or
 * 1/X) built by ds_deconv_inverse; ir = irfft(rfft(y, n_fft) * r, n_fft),
 * first n_out samples stored.                                                */
int ds_rfft_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ld, int64_t n_samples,
                int n_fft, float scale, ds_c32* spec_dev);
int ds_rfft(ds_ctx* ctx, const float* x, int n_ch, int64_t n_samples, int n_fft,
            float scale, ds_c32* spec);
/* r[c][b] = eps ? conj(X)/(|X|^2+eps[b]) : 1/X   (eps_dev may be NULL)        */
int ds_deconv_inverse_dev(ds_ctx* ctx, const ds_c32* xspec_dev /*B x n_ch*/, int n_ch,
                          int n_bins, const float* eps_dev, ds_c32* r_dev /*n_ch x B*/);
int ds_deconv_dev(ds_ctx* ctx, const float* y_dev, int n_items, int n_ch, int64_t ld,
                  int64_t n_samples, int n_fft, const ds_c32* r_dev, int r_per_channel,
                  int64_t n_out, int64_t ld_out, float* ir_dev);
int ds_deconv(ds_ctx* ctx, const float* y, int n_items, int n_ch, int64_t n_samples,
              int n_fft, const ds_c32* r, int r_per_channel, int64_t n_out, float* ir);

/* ---- FIR filtering by FFT block convolution: replaces _lfilter_fir,
 * classes/filter_helpers.py:454-503 (scipy.signal.oaconvolve(...)[:N]) and the
 * filter loop of _filterbank_on_signal, :385-451.
 * y = (x * taps_k)[0:N] for each of n_filt filters of n_taps taps
 * (taps[k*n_taps + t]); DS_FB_PARALLEL: y[(k*n_ch + c)*ld_y + n];
 * DS_FB_SUMMED / DS_FB_SEQUENTIAL: y[c*ld_y + n].
 * Up to 8193 taps: LDS-resident blocks of <= 16384 points; longer filters (to
 * 2^23 + 1 taps): overlap-save on the four-step FFT.  Filter state (zi) and
 * zero-phase filtering are built on this call by the host shim: the full
 * convolution is this call over the signal followed by n_taps - 1 zeros.      */
int ds_fir_ola_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx,
                   int64_t n_samples, const float* taps_dev, int n_filt, int n_taps,
                   int mode, float* y_dev, int64_t ld_y);
int ds_fir_ola(ds_ctx* ctx, const float* x, int n_ch, int64_t n_samples,
               const float* taps, int n_filt, int n_taps, int mode, float* y);

/* ---- IIR filtering: cascades of second-order sections, float64 recursion: replaces scipy.signal.sosfilt /
 * lfilter in _filter_on_signal (classes/filter_helpers.py:207-280), the IIR branch of _filter_on_signal_ba
 * (:288-382) and the filter loop of _filterbank_on_signal (:385-451) for IIR filters.
 * sos [n_filt][n_sec][6] float64, host pointer: each row b0 b1 b2 a0 a1 a2 (a0 != 0; the rows are divided by it),
 * each filter a cascade of n_sec sections in transposed direct form II -- what sosfilt computes.  Filters with
 * fewer sections are padded by the caller with the identity section 1 0 0 1 0 0.
 * zi / zf [n_filt][n_sec][2][n_ch] float64 (sosfilt's (n_sec, 2, channels) state per filter): the initial state
 * (NULL: zero) and the final state after the last sample (NULL: not wanted).
 * mode DS_FB_PARALLEL: every filter on every channel, y[k] per filter; DS_FB_SUMMED: the sum over the filters;
 * DS_FB_SEQUENTIAL: one cascade of all n_filt * n_sec sections (sos, zi and zf read as [1][n_filt * n_sec]...).
 * One cascade holds at most 32 sections (DS_ERR_UNSUP above); n_filt * n_ch <= 65535.  The filters must be
 * stable (every pole inside the unit circle): the time-parallel carry is exact only for them.
 * ds_iir_sos: host pointers in the reference's layouts, x (n_samples, n_ch) float64, y (n_filt or 1, n_samples,
 * n_ch) float64.
 * ds_iir_sos_dev: device-resident planar float32 samples, x_dev[c*ldx + n]; DS_FB_PARALLEL:
 * y_dev[(k*n_ch + c)*ld_y + n], otherwise y_dev[c*ld_y + n]; zi_dev / zf_dev device pointers (or NULL);
 * sos stays a host pointer.  The recursion itself is float64 on both entries.                              */
int ds_iir_sos(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, const double* sos, int n_filt,
               int n_sec, const double* zi, int mode, double* y, double* zf);
int ds_iir_sos_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, const double* sos,
                   int n_filt, int n_sec, const double* zi_dev, int mode, float* y_dev, int64_t ld_y,
                   double* zf_dev);

/* ---- IIR filtering with COMPLEX coefficients (csrc/kernels_ciir.hpp): what scipy.signal.sosfilt computes for a complex
 * sos array and real samples -- the four cascaded complex one-pole sections of a gammatone band
 * (filterbanks/filterbanks.py:217-303).  The recursion, the states and the carry over time are complex float64.
 * sos [n_filt][n_sec][6] complex128 (interleaved doubles), host pointer, rows b0 b1 b2 a0 a1 a2 (a0 != 0), identity-padded
 * by the caller; zi / zf [n_filt][n_sec][2][n_ch] complex128 or NULL; x (n_samples, n_ch) float64 REAL, host pointer.
 * The output is two float64 planes in the reference's layout (n_filt, n_samples, n_ch): y_re and y_im; y_im may be NULL
 * (the real part only).  Every filter runs on every channel (Parallel); there is no summed or sequential mode.
 * Bounds: one cascade holds at most 16 sections (CIIR_MAX_SEC of the kernels; DS_ERR_UNSUP above); n_filt * n_ch <= 65535;
 * DS_ERR_NOMEM, before anything is uploaded, when the device has not the memory free.  The filters must be stable.   */
int ds_iir_sos_c128(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, const double* sos, int n_filt, int n_sec,
                    const double* zi, double* y_re, double* y_im, double* zf);

/* ---- structure filters (csrc/kernels_sfilt.hpp): the sample loops of the reference's LatticeLadderFilter
 * (classes/lattice_ladder_filter.py), WarpedFIR / WarpedIIR (classes/warped_filters.py) and KautzFilter
 * (classes/kautz_filter.py) as float64 recursions over d <= 64 real state values, time-parallel with the carry of
 * ds_iir_sos.  kind and the packed float64 coefficient array coef (host pointer), `aux` a count beside d:
 *   DS_SFILT_FIR_LATTICE  k[d]                                         state: the reference's (len(k), channels)
 *   DS_SFILT_IIR_LATTICE  k[d], c[d + 1]                               state: (len(k), channels)
 *   DS_SFILT_SOS_LATTICE  per section k0 k1 c0 c1 c2, d = 2 sections   state: (sections, 2, channels)
 *   DS_SFILT_WARPED_FIR   lambda, b[d]                                 state: WarpedFIR.buffer (len(b), channels)
 *   DS_SFILT_WARPED_IIR   lambda, b[d] zero-padded to d = max(len(a), len(b)), sigma[0 .. aux], aux = len(a)
 *                                                                      state: WarpedIIR.buffer (d, channels)
 *   DS_SFILT_KAUTZ        aux real poles: pole, normalisation, weight each; then (d - aux) / 2 pole pairs: q, r, the two
 *                         normalisations, the two weights each.  State: one direct-form-II value w[n-1] per real pole,
 *                         (w[n-1], w[n-2]) per pair, shared by the tap filters and the all-pass of that pole.
 * zi / zf [d][n_ch] float64, HOST pointers on both entries: the initial state (NULL: zero) and the state after the last
 * sample (NULL: not wanted).  Bounds: d <= 64 and n_ch <= 65535 (DS_ERR_UNSUP above); the largest magnitude in
 * Phi = A^32 and Phi^64 (A the zero-input state transition) at most 30 for the warped IIR filter and 1e6 for the others
 * (MAX_GAIN_WARPED_IIR, MAX_GAIN of the kernels), DS_ERR_UNSUP above -- that refuses unstable and too ill-conditioned
 * recursions; DS_ERR_NOMEM, before anything is uploaded, when the device has not the memory free.
 * ds_sfilt: x and y (n_samples, n_ch) float64 host arrays.
 * ds_sfilt_dev: device-resident planar float32 samples x_dev[c*ldx + n] -> y_dev[c*ld_y + n]; the recursion itself is
 * float64 on both entries.                                                                                        */
#define DS_SFILT_FIR_LATTICE 0
#define DS_SFILT_IIR_LATTICE 1
#define DS_SFILT_SOS_LATTICE 2
#define DS_SFILT_WARPED_FIR 3
#define DS_SFILT_WARPED_IIR 4
#define DS_SFILT_KAUTZ 5
int ds_sfilt(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, int kind, const double* coef, int d, int aux,
             const double* zi, double* y, double* zf);
int ds_sfilt_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, int kind, const double* coef,
                 int d, int aux, const double* zi, float* y_dev, int64_t ld_y, double* zf);

/* ---- realtime filters (csrc/kernels_rtfilt.hpp): the sample loops of the reference's StateVariableFilter
 * (classes/sv_filter.py), IIRFilter (classes/iir_filter_realtime.py), ParallelFilter (classes/parallel_filter.py) and
 * StateSpaceFilter (classes/state_space_filter.py) as float64 recursions over d <= 64 real state values, time-parallel
 * with the carry of ds_iir_sos.  kind and the packed float64 coefficient array coef (host pointer), `aux` a count beside d:
 *   DS_RTFILT_SVF          g, resonance, 1 / (1 + resonance g + g^2); d = 2, aux = 0     state: the reference's (2, channels)
 *   DS_RTFILT_TDF2         b[d + 1], a[d + 1], zero-padded to the order d, a[0] = 1       state: (order, channels)
 *   DS_RTFILT_PARALLEL     per section b0 b1 b2 a1 a2 (a0 = 1): aux sections, d = 2 aux   state: sosfilt's (z1, z2) per section
 *   DS_RTFILT_STATE_SPACE  A[d][d] row-major, B[d], C[d], D                               state: StateSpaceFilter.x (d, channels)
 * The state-variable filter writes FOUR bands (low, high, band, all-pass), the others one.  A parallel filter's sections
 * all read the input delayed by `delay` samples (zeros in front) and their outputs are added, in section order, to the
 * FIR part's sample sum_i fir[i] x[n - i] (fir NULL or n_fir = 0: to zero); delay, fir and aux are 0 / NULL for the other
 * kinds (DS_ERR_ARG otherwise).  zi / zf [d][n_ch] float64, HOST pointers on both entries: the initial state (NULL:
 * zero) and the state after the last sample (NULL: not wanted).  Bounds: d <= 64, n_ch <= 65535 (DS_ERR_UNSUP above); the
 * largest magnitude in Phi = A^32 and Phi^64 (A the zero-input state transition) at most 30 for DS_RTFILT_TDF2 and
 * DS_RTFILT_STATE_SPACE and 1e6 for the other two (MAX_GAIN_COMPANION, MAX_GAIN of the kernels), DS_ERR_UNSUP above
 * (DESIGN section 26); the FIR part's bounds are ds_rtfir's; DS_ERR_NOMEM, before anything is uploaded, when the device
 * has not the memory free.
 * ds_rtfilt: x (n_samples, n_ch) and y (bands, n_samples, n_ch) float64 host arrays.
 * ds_rtfilt_dev: device-resident planar float32 samples x_dev[c*ldx + n] -> y_dev[(band*n_ch + c)*ld_y + n]; the
 * recursion itself is float64 on both entries.
 *
 * ds_rtfir / ds_rtfir_dev: the direct float64 FIR sum y[n] = b[0] x[n] + sum_{i < order} b[i + 1] x[n - 1 - i], order =
 * n_taps - 1, one fused multiply-add per term in that order (two calls give the same bits).  hist [n_ch][order] float64,
 * host pointer: the samples before the first one, x[-order] first (NULL: zeros).  Bounds (DS_ERR_UNSUP above): n_taps <=
 * 4096, n_samples * n_ch * n_taps <= 2^40, n_ch <= 65535.  Layouts as ds_rtfilt / ds_rtfilt_dev with one band.         */
#define DS_RTFILT_SVF 0
#define DS_RTFILT_TDF2 1
#define DS_RTFILT_PARALLEL 2
#define DS_RTFILT_STATE_SPACE 3
int ds_rtfilt(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, int kind, const double* coef, int d, int aux,
              int64_t delay, const double* fir, int n_fir, const double* zi, double* y, double* zf);
int ds_rtfilt_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, int kind, const double* coef,
                  int d, int aux, int64_t delay, const double* fir, int n_fir, const double* zi, float* y_dev, int64_t ld_y,
                  double* zf);
int ds_rtfir(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, const double* b, int n_taps, const double* hist,
             double* y);
int ds_rtfir_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, const double* b, int n_taps,
                 const double* hist, float* y_dev, int64_t ld_y);

/* ---- per-channel sums over a pair of signals, float64, fixed summation order (csrc/kernels_dist.hpp): the device part
 * of distances.snr and distances.si_sdr (distances/_distances.py:64-101).  par (n_ch, 3) float64, host pointer, holds
 * alpha, mu_a, mu_b per channel (NULL: zeros); out (n_ch, 6) float64, host pointer, receives
 *   sum (a - mu_a)^2, sum (b - mu_b)^2, sum a b, sum a, sum b, sum (alpha a - b)^2      -- the last one term by term.
 * a (n, n_ch_a) and b (n, n_ch_b) float64 host arrays, or for the _dev entry planar fp32 on the device (channel ch at
 * a_dev + ch lda); a side with ONE channel is paired with every channel of the other; n_ch = max(n_ch_a, n_ch_b).  */
int ds_pair_moments(ds_ctx* ctx, const double* a, int n_ch_a, const double* b, int n_ch_b, int64_t n, const double* par,
                    double* out);
int ds_pair_moments_dev(ds_ctx* ctx, const float* a_dev, int n_ch_a, int64_t lda, const float* b_dev, int n_ch_b,
                        int64_t ldb, int64_t n, const double* par, double* out);

/* ---- frequency-weighted segmental SNR: distances.fw_snr_seg (distances/distances.py:275-387, _fw_snr_seg_per_channel,
 * distances/_distances.py:104-195) in one call.  Both signals go through the gammatone bank sos [n_band][n_sec][6]
 * complex128 (ds_iir_sos_c128's recursion, real part only); the band signals stay in HBM as float64.  Frames of
 * window_length samples (even; the window is window[window_length], host float64), hop window_length / 2, zeros past the
 * signal's end, n_frames = ceil(n / hop).  Per (frame, band, channel) ONE complex float64 transform of x_band w + i
 * xhat_band w gives both spectra; per (frame, channel) the bands' log10(X^2 / (X - Xhat + 1e-30)^2) |X|^gamma are summed,
 * weighted, averaged over the bins 0 .. window_length / 2 and clipped to [snr_lo_db, snr_hi_db]; out[n_ch] is the mean
 * over the frames.  Fixed summation order: repeats give the same bits.  A frame whose spectrum sums to zero gives NaN, as
 * in the reference.  x has n_ch channels or ONE (paired with every channel of xhat).  The frames are walked in chunks of
 * chunk_frames (0: 32), fewer where (chunk x bands x channels) would pass 65535 transform columns.
 * Bounds: window_length <= 16384, n_band * n_ch <= 65535, n_sec <= 16 (DS_ERR_UNSUP); DS_ERR_NOMEM, before anything is
 * uploaded, when the device has not the memory free.
 * ds_fw_snr_seg: host (n, channels) float64; ds_fw_snr_seg_dev: planar fp32 on the device, channel ch at x_dev + ch ldx. */
int ds_fw_snr_seg(ds_ctx* ctx, const double* x, int n_ch_x, const double* xhat, int n_ch, int64_t n, const double* sos,
                  int n_band, int n_sec, const double* window, int window_length, double snr_lo_db, double snr_hi_db,
                  double gamma, int chunk_frames, double* out);
int ds_fw_snr_seg_dev(ds_ctx* ctx, const float* x_dev, int n_ch_x, int64_t ldx, const float* xhat_dev, int n_ch, int64_t ldxh,
                      int64_t n, const double* sos, int n_band, int n_sec, const double* window, int window_length,
                      double snr_lo_db, double snr_hi_db, double gamma, int chunk_frames, double* out);

/* ---- fractional delays and their weighted sums, float64 arithmetic: replaces the reference's fractional_delay
 * (standard/latency_delay.py:159-285, filter from standard/_standard_backend.py:259-321, :430-492) and the loops of
 * MonopoleSource.get_signals_on_array, mix_sources_on_array and BeamformerDASTime (beamforming/beamforming.py:
 * 1317-1512).  Computes, for 0 <= g < n_rows and 0 <= t < out_len,
 *     y[g, t] = sum_{j < n_terms} w[g,j] sum_{k <= order} h(frac[g,j])[k] x_{src[g,j]}[t - shift[g,j] - k]
 * with x_c[n] = 0 outside [0, src_len[c]).  h(f) is the reference's Kaiser-windowed sinc for the fractional delay f
 * (0 <= f < 1, side lobe parameter beta = _kaiser_window_beta(...)); a term with frac < 0 is a pass-through, the
 * single unit tap of a delay of exactly 0.  shift may be negative, |shift| <= INT64_MAX / 4 (DS_ERR_ARG beyond).  The per-term arrays src (int), shift (int64),
 * frac and weight (float64) are host pointers laid out [n_rows][n_terms]; src_len is a host array [n_src].
 * peak (host, [n_rows], or NULL) receives each row's max |y| as computed, before any rounding of the output type;
 * y may be NULL when only the peaks are wanted.  Orders 1 to 255 and at most 262140 rows: DS_ERR_UNSUP beyond.
 * ds_delay_sum: x (n_x, n_src) float64 host (the reference's (samples, channels)), src_len[c] <= n_x;
 * y (out_len, n_rows) float64 host.
 * ds_delay_sum_dev: x_dev planar float32 x_dev[c*ldx + n], src_len[c] <= ldx; y_dev[g*ld_y + t] float32.          */
int ds_delay_sum(ds_ctx* ctx, const double* x, int n_src, int64_t n_x, const int64_t* src_len, int n_rows,
                 int n_terms, const int* src, const int64_t* shift, const double* frac, const double* weight,
                 int order, double beta, int64_t out_len, double* y, double* peak);
int ds_delay_sum_dev(ds_ctx* ctx, const float* x_dev, int n_src, int64_t ldx, const int64_t* src_len, int n_rows,
                     int n_terms, const int* src, const int64_t* shift, const double* frac, const double* weight,
                     int order, double beta, int64_t out_len, float* y_dev, int64_t ld_y, double* peak);

/* ---- continuous wavelet transform: replaces the loop of the reference's transforms.cwt (transforms/transforms.py:
 * 687-760) and _squeeze_scalogram (transforms/_transforms.py:227-301).  Row f of the scalogram is the "same"-mode
 * convolution (scipy.signal.oaconvolve(..., mode="same")) of every channel with wavelet f:
 *     S[f, n, c] = sum_k w_f[k] x_c[n + (L_f - 1) / 2 - k],   0 <= n < n_samples,
 * computed in fp32 / complex64 by overlap-save in power-of-two size classes (csrc/kernels_cwt.hpp).  The wavelets are
 * host arrays: taps holds all of them back to back as interleaved complex64 (wavelet f: tap_len[f] values, already
 * normalised by the caller), tap_len is [n_freq].  1 <= L_f <= 2^18 (DS_ERR_UNSUP beyond, before any launch).
 * ds_cwt: x (n_samples, n_ch) float64 host, the reference's layout; out (n_freq, n_samples, n_ch) host, complex64
 *   (out_f64 = 0) or complex128.
 * ds_cwt_dev: x_dev planar float32 x_dev[c*ldx + n]; channels[n_out_ch] (host) picks and orders the channels;
 *   out_dev (n_freq, n_samples, n_out_ch) complex64 on the device.
 * ds_cwt_squeeze_dev: synchrosqueezing of a device scalogram s_dev (n_freq, n_samples, n_ch) complex64 into out_dev
 *   of the same shape, complex128, in float64 arithmetic: the gradient along time (np.gradient), the phase
 *   transform |Im(g / S)| / (2 pi) fs where |S|^2 > 1e-40 (0 elsewhere), the first nearest of freqs[] (host, the
 *   caller's order) and a skip beyond delta_f[f]; norm (host, [n_freq], or NULL) scales each summed row.
 *   n_samples >= 2.                                                                                                  */
int ds_cwt(ds_ctx* ctx, const double* x, int n_ch, int64_t n_samples, int n_freq, const int64_t* tap_len,
           const float* taps, int out_f64, void* out);
int ds_cwt_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, const int* channels,
               int n_out_ch, int n_freq, const int64_t* tap_len, const float* taps, float* out_dev);
int ds_cwt_squeeze_dev(ds_ctx* ctx, const float* s_dev, int n_freq, int64_t n_samples, int n_ch, const double* freqs,
                       const double* delta_f, const double* norm, double fs, double* out_dev);

/* ---- fractional-octave smoothing, float64: replaces the reference's _fractional_octave_smoothing (helpers/
 * smoothing.py:9-129) and the magnitude / unwrapped-phase smoothing around it in Signal.get_spectrum (classes/
 * signal.py:913-928) and Spectrum.apply_octave_smoothing (classes/spectrum.py:805-869).  v, out: (n_bins, n_ch) host
 * arrays, channel fastest.  k_log (host, [n_bins]): the logarithmic axis n_bins ** (arange(n_bins) / (n_bins - 1)) of
 * linearly spaced bins, computed by the caller; strictly ascending with k_log[0] <= 1 and k_log[n_bins - 1] >=
 * n_bins (DS_ERR_ARG otherwise).  The data goes to that axis with scipy's PchipInterpolator (knots 1 .. n_bins), is
 * smoothed, and comes back by linear interpolation.  k_log = NULL: the bins are logarithmic already, both
 * interpolations are skipped.  window (host, [n_window], any non-zero sum: normalised to unit sum here): the data is
 * edge-padded by n_window / 2 in front and n_window / 2 - (1 - n_window % 2) behind and convolved in valid mode,
 *     out[i] = sum_k window[k] v[clamp(i + n_window - 1 - k - n_window / 2, 0, n_bins - 1)] / sum(window),
 * by direct summation.  clip != 0: negative results become 0.  n_bins * n_window * n_ch beyond the work bound of
 * csrc/size_guards.hpp: DS_ERR_UNSUP, before any launch.
 * ds_octave_smooth_complex: z, out (n_bins, n_ch) complex128 (interleaved doubles); |z| (clipped if clip_magnitude)
 * and numpy.unwrap(angle(z)) along the bins are smoothed as above and recombined as mag * exp(i phase); the work
 * counts 2 n_ch channels.                                                                                       */
int ds_octave_smooth(ds_ctx* ctx, const double* v, int64_t n_bins, int n_ch, const double* k_log, const double* window,
                     int64_t n_window, int clip, double* out);
int ds_octave_smooth_complex(ds_ctx* ctx, const double* z, int64_t n_bins, int n_ch, const double* k_log,
                             const double* window, int64_t n_window, int clip_magnitude, double* out);

/* ---- direct sums, float64 (csrc/kernels_direct.hpp) --------------------------------------------------------------
 * ds_dft: out[k][c] = sum_n x[n][c] w_k,c[n] exp(-2 pi i freqs_hz[k] n / fs_hz) for ANY frequencies (0, negative and
 * beyond fs / 2 included) -- transforms.dft of the reference (transforms/transforms.py:1286-1327).  x (n_samples, n_ch)
 * float64 and out (n_freq, n_ch) complex128 are host arrays.  alpha NULL: w = 1.  Otherwise the Gaussian window of
 * transfer_functions.window_frequency_dependent (transfer_functions/transfer_functions.py:1288-1377):
 * w_k,c[n] = exp(alpha[k] * -0.5 ((n - peak[c]) / half)^2), alpha [n_freq], peak [n_ch] sample indices; terms whose
 * weight is below 2^min_weight_log2 are skipped per (bin, channel) (-70 keeps the skipped sum 12 orders below the
 * result; -INFINITY keeps every term).  ds_dft_dev: the same on device-resident planar float32 samples
 * (x_dev[c * ldx + n]), widened on load.  n_freq = 0 or n_ch = 0: nothing is launched.  The terms summed -- n_freq *
 * n_samples * n_ch, or the kept ranges of the windowed form -- are bounded per call (csrc/size_guards.hpp):
 * DS_ERR_UNSUP beyond, before anything is uploaded.
 * ds_complex_smooth: the band sums of transfer_functions.complex_smoothing (:1788-1876) and the domain transforms
 * around them.  z, out (n_bins, n_ch) complex128 on the host.  Per bin i the caller gives the band [ind_low, ind_high)
 * clipped to the spectrum, its unclipped window_length and pass (non-zero: the bin is copied); the device evaluates
 * W_i[m] = interp(10^linspace(log10 3, 0, window_length)[m] - 2, window_x, window_y) on the n_window-point prototype,
 * and out[i] = sum_m W_i[m] q[ind_low + m] / sum_m W_i[m] with q the domain's quantity.  The band lengths x n_ch are
 * bounded as above.                                                                                               */
#define DS_SMOOTH_REAL_IMAGINARY     0
#define DS_SMOOTH_POWER_PHASE        1
#define DS_SMOOTH_MAGNITUDE_PHASE    2
#define DS_SMOOTH_POWER              3
#define DS_SMOOTH_MAGNITUDE          4
#define DS_SMOOTH_EQUIVALENT_COMPLEX 5
int ds_dft(ds_ctx* ctx, const double* x, int64_t n_samples, int n_ch, const double* freqs_hz, int64_t n_freq,
           double fs_hz, const double* alpha, const int64_t* peak, double half, double min_weight_log2, double* out);
int ds_dft_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, const double* freqs_hz,
               int64_t n_freq, double fs_hz, const double* alpha, const int64_t* peak, double half,
               double min_weight_log2, double* out);
int ds_complex_smooth(ds_ctx* ctx, const double* z, int64_t n_bins, int n_ch, const int32_t* ind_low,
                      const int32_t* ind_high, const int32_t* window_length, const int32_t* pass,
                      const double* window_x, const double* window_y, int n_window, int domain, double* out);

/* ---- complex128 transforms of any length along axis 0, and what the reference builds on them (csrc/kernels_fft64.hpp):
 * transforms.hilbert / cepstrum / from_complex_cepstrum (transforms/transforms.py:59-110, 763-809), the real-cepstrum
 * minimum-phase equivalent (helpers/minimum_phase.py:8-79) and the group delay from the unwrapped phase
 * (standard/_standard_backend.py:37-63).  Host pointers, float64 / complex128 (interleaved doubles) arrays in the
 * reference's (rows, channels) C order; everything between the upload and the download stays on the device.
 * Lengths: powers of two up to 2^22, every other length up to 2^21, DS_ERR_UNSUP beyond; DS_ERR_NOMEM, before anything
 * is uploaded, when the device has not the memory free that the call needs.
 * The generic transform: `in` is (n_in, n_ch) float64 or, with in_complex, complex128; it is zero-padded or cropped to
 *   n_fft rows; out is (n_fft, n_ch) complex128; the inverse divides by n_fft as numpy does.
 * The analytic signal, out (n, n_ch) complex128.  The cepstrum ifft(log(fft(x))), or with complex_cepstrum = 0
 *   ifft(log|fft(x)|), out (n, n_ch) complex128; and its way back real(ifft(exp(fft(cepstrum)))), out (n, n_ch) float64.
 * The minimum-phase equivalent of x zero-padded (or cropped) to n_fft rows, by `output`: its spectrum (n_fft, n_ch)
 *   complex128; the phase of its bins 0 .. n_fft / 2, float64; its impulse response, the first n_out rows, float64; its
 *   group delay -gradient(unwrap(phase)) / (2 pi delta_f) on the same n_fft / 2 + 1 bins, float64.
 * The group delay of x itself from the phase of its n / 2 + 1 non-negative bins, float64.                          */
#define DS_MIN_PHASE_SPECTRUM 0
#define DS_MIN_PHASE_PHASE 1
#define DS_MIN_PHASE_IR 2
#define DS_MIN_PHASE_GROUP_DELAY 3
int ds_fft_c128(ds_ctx* ctx, const double* in, int in_complex, int64_t n_in, int n_ch, int64_t n_fft, int inverse,
                double* out);
int ds_hilbert(ds_ctx* ctx, const double* x, int64_t n, int n_ch, double* out);
int ds_cepstrum(ds_ctx* ctx, const double* x, int64_t n, int n_ch, int complex_cepstrum, double* out);
int ds_from_cepstrum(ds_ctx* ctx, const double* cepstrum, int64_t n, int n_ch, double* out);
int ds_min_phase(ds_ctx* ctx, const double* x, int64_t n, int n_ch, int64_t n_fft, int output, int64_t n_out,
                 double delta_f, double* out);
int ds_group_delay_phase(ds_ctx* ctx, const double* x, int64_t n, int n_ch, double delta_f, double* out);

/* ---- latency estimation by cross-correlation (csrc/kernels_latency.hpp on the transforms above): standard.latency of
 * the reference (standard/latency_delay.py:15-156; _latency, standard/_standard_backend.py:14-34; _fractional_latency,
 * _get_fractional_impulse_peak_index, _get_correlation_of_latencies, helpers/latency.py:10-149, 218-265) and the latency
 * removal of group_delay (transfer_functions.py:908-914).  Host pointers, float64 in (rows, channels) C order.
 * ds_latency: a (n_a, n_ch) is the delayed signal, b (n_b, n_ch_b) the original, n_ch_b = n_ch or 1 (one column for
 *   every pair).  Channel c of scipy's full-mode correlate(b, a), L = n_a + n_b - 1 rows, is formed on the device and stays
 *   there.  peaks [n_ch], int64: the row of the largest magnitude, the lowest row among equal ones; the lag is
 *   n_a - 1 - peak.  With polynomial_points p > 0: window [2] = (lo, M), the rows [max(min peak - 200, 0),
 *   min(max peak + 200, L)) shared by all channels, and near [n_ch][2 p + 2], the values imag(hilbert(window))[d - p ..
 *   d + p + 1] around each channel's own peak row d = peak - lo, NaN for a row outside the window.  pearson (or NULL)
 *   [n_ch][n_cand]: Pearson's r of the pair (b column j, a column j) at the integer lags n_a - 1 - peak' + (-1, 0, 1)
 *   (n_cand = 3; p = 0: the lag itself, n_cand = 1), with peak' that of column j or, reverse_pairs, of column
 *   n_ch - 1 - j; NaN where fewer than two samples overlap or a channel is constant.
 *   b = NULL: no correlation, the peaks, window and values are those of a itself; pearson must be NULL.
 *   DS_ERR_UNSUP: L above 2^22, more than 65535 columns (n_ch + n_ch_b), p above 16, and -- found after the peak search,
 *   with nothing launched after it; window is written -- a window M above 2^21 that is no power of two.  DS_ERR_NOMEM
 *   before anything is uploaded, counted for the widest window (M = L).
 * ds_lag_pearson: Pearson's r per row of rows [n_rows][3] = (column of t, column of o, lag), int64: lag > 0 drops the
 *   first lag samples of o's column, otherwise the first -lag of t's; both are cut to the shorter; out [n_rows].
 * ds_group_delay_phase_lat: ds_group_delay_phase with the phase wrap(angle + 2 pi f latency_samples[c] / fs),
 *   f = k delta_f, wrap(x) = (x + pi) mod 2 pi - pi, before the unwrap.                                             */
int ds_latency(ds_ctx* ctx, const double* a, int64_t n_a, int n_ch, const double* b, int64_t n_b, int n_ch_b,
               int polynomial_points, int reverse_pairs, int64_t* peaks, int64_t* window, double* near,
               double* pearson);
int ds_lag_pearson(ds_ctx* ctx, const double* t, int64_t n_t, int n_ch_t, const double* o, int64_t n_o, int n_ch_o,
                   const int64_t* rows, int n_rows, double* out);
int ds_group_delay_phase_lat(ds_ctx* ctx, const double* x, int64_t n, int n_ch, double delta_f,
                             const double* latency_samples, double fs, double* out);

/* ---- linear prediction per (frame, channel) pair (csrc/kernels_lpc.hpp): transforms.lpc of the reference
 * (transforms/transforms.py:1199-1283) with its estimators (helpers/ar_estimation.py:6-205) and its framing and
 * overlap-add (standard/_framed_signal_representation.py:9-137), float64 on the device.
 * Frames: n_frames = ceil(n_samples / hop); frame f covers the samples f hop .. f hop + window_length - 1, zeros past
 *   the signal's end, times window[window_length] (host, float64).  Framed and windowed inside the kernel.
 * The estimate: x is host (n_samples, n_ch) float64, or for the _dev entry planar fp32 on the device, channel c at
 *   x_dev + c ldx, widened on load.  method DS_LPC_YULE_WALKER: the biased autocorrelation r[k] = sum x[n] x[n + k] /
 *   window_length, k = 0 .. order, then the Levinson-Durbin recursion (ar_estimation.py:28-60); var is the final
 *   prediction error.  DS_LPC_BURG: Burg's method with eps(float64) added to the denominator (ar_estimation.py:162-205);
 *   var is its running denominator `den`, divided by nothing, as the reference returns it.  a: host (order + 1, n_frames,
 *   n_ch) float64 with a[0] = 1 (the reference pads its Burg result with zero rows up to window_length + 1: the caller's
 *   business); var: host (n_frames, n_ch).  A frame that is all zeros gives a[1 ..] = var = NaN with Yule-Walker and
 *   a = [1, 0, ...], var = 0 with Burg, as IEEE division gives them in the reference.  *singular is 1 when the
 *   prediction error of any pair was <= 0 after any order (where the reference raises "Singular Matrix"; Burg never
 *   sets it), else 0; a and var are written either way.
 * The recursion alone on a host (order + 1, n_cols) autocorrelation: a (order + 1, n_cols), var (n_cols), *singular.
 * The synthesis: scipy's lfilter([1], a[:, f, c], sources[:, f, c]) from zero state for every pair -- a and sources are
 *   host (order + 1, n_frames, n_ch) and (window_length, n_frames, n_ch) -- then the reference's overlap-add: frames
 *   times the window, added at hop spacing, over the envelope sum window^2 clipped below at 1e-4, padded with zeros or
 *   trimmed to n_out samples; y is host (n_out, n_ch).
 * Bounds: 1 <= order < window_length and hop >= 1 (DS_ERR_ARG); window_length <= 8192, order <= 255, fewer than 2^31
 *   pairs and frames x channels x window_length x (order + 1) within the work bound of csrc/size_guards.hpp
 *   (DS_ERR_UNSUP); DS_ERR_NOMEM, before anything is uploaded, when the device has not the memory free.           */
#define DS_LPC_YULE_WALKER 0
#define DS_LPC_BURG 1
int ds_lpc(ds_ctx* ctx, const double* x, int64_t n_samples, int n_ch, const double* window, int window_length,
           int64_t hop, int order, int method, double* a, double* var, int* singular);
int ds_lpc_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_samples, const double* window,
               int window_length, int64_t hop, int order, int method, double* a, double* var, int* singular);
int ds_levinson(ds_ctx* ctx, const double* r, int order, int64_t n_cols, double* a, double* var, int* singular);
int ds_lpc_synth(ds_ctx* ctx, const double* a, const double* sources, const double* window, int window_length,
                 int64_t n_frames, int n_ch, int64_t hop, int order, int64_t n_out, double* y);

/* ---- the all-pass table of frequency warping and the Laguerre transform (csrc/kernels_warp.hpp, csrc/warp_plan.hpp):
 * transforms.warp and transforms.laguerre of the reference (transforms/transforms.py:955-1130,
 * transforms/_transforms.py:386-428), float64 on the device.  With a given first row row0[n_out] and first column
 * col0[n_in] (host, float64; c[0][0] is taken from col0[0]) the table is
 *   c[i][j] = p c[i-1][j] + c[i-1][j-1] + q c[i][j-1]   (i, j >= 1),     out[j][ch] = sum_i c[i][j] x[i][ch].
 *   warp(lambda):    p = -lambda, q = lambda, row0 = the unit pulse, col0[i] = (-lambda)^i; i is the input sample.
 *   laguerre(f):     p = -f, q = f, col0[i] = sqrt(1 - f^2) (-f)^i, row0[j] = sqrt(1 - f^2) f^j.
 * x is host (n_in, n_ch) float64, or for the _dev entry planar fp32 on the device, channel ch at x_dev + ch ldx, widened on
 * load; out is host (n_out, n_ch) float64.  n_in and n_out are independent.  The table is computed tile by tile, one launch
 * per tile anti-diagonal on the context's stream, and summed in a fixed order: repeats give the same bits, and with
 * p = q = 0 and identity boundaries out equals x bit for bit.
 * Bounds: sizes >= 1 and finite p, q (DS_ERR_ARG); n_in, n_out <= 131072, n_ch <= 65536 and n_in x n_out x ceil(n_ch / 4)
 *   within the work bound of csrc/size_guards.hpp (DS_ERR_UNSUP); DS_ERR_NOMEM, before anything is uploaded, when the
 *   device has not the memory free.                                                                                    */
int ds_allpass_table(ds_ctx* ctx, const double* x, int64_t n_in, int n_ch, double p, double q, const double* row0,
                     const double* col0, int64_t n_out, double* out);
int ds_allpass_table_dev(ds_ctx* ctx, const float* x_dev, int n_ch, int64_t ldx, int64_t n_in, double p, double q,
                         const double* row0, const double* col0, int64_t n_out, double* out);

/* ---- shoebox room simulation (csrc/kernels_room.hpp): the image-source sum of room_acoustics.generate_synthetic_rir
 * (room_acoustics/_room_acoustics.py:162-269) and the modal sum of ShoeboxRoom.get_analytical_transfer_function
 * (:554-685) of the reference, float64 on the device.
 * ds_room_ism: the cells (l, m, n), each index -limit .. limit, in row-major order, eight sources per cell in the
 *   reference's order u = 000 001 010 100 011 101 110 111 (ux uy uz).  Source (cell, u) lies at
 *   pos = (1 - 2u) src + 2 l dim - rec per axis, d = sqrt((x^2 + y^2) + z^2), falls into sample int(d / c sr + 0.5) and adds
 *   ((pw[0][|l - ux|] pw[1][|m - uy|]) pw[2][|n - uz|]) ((pw[3][|l|] pw[4][|m|]) pw[5][|n|]) / (4 pi d) there, every
 *   operation rounded on its own.  Inside one cell a source whose sample equals that of a later source of the cell
 *   is dropped, as the reference's fancy-index += drops it; sources at or beyond n_out are dropped.  pw is host
 *   (n_band, 6, limit + 2): the powers beta^k, k = 0 .. limit + 1, of the walls south, west, floor, north, east,
 *   ceiling per band; all bands share the enumeration.  out: host (n_band, n_out).  Per sample the kept sources are
 *   added in the reference's loop order, so repeats give the same bits.  The kept sources' ids are listed l slab by
 *   l slab, a slab's list within max_list_bytes (<= 0: the bound of csrc/size_guards.hpp).
 *   The caller guarantees what the reference's buffer guarantees: every sample index is below 2^31 (backend.py raises
 *   the reference's IndexError first) and src != rec.
 * ds_room_modal_tf: p[f] = sum_n weight[n] / (omega_n[n]^2 + 2j eta[n] omega_n[n] - omega2[f]) over the table's n_modes
 *   entries in table order, one writer per frequency; p: host (n_freq) complex128.
 * Bounds: limit >= 0, n_out, n_band, n_modes, n_freq >= 1, positive finite dim, c, sr (DS_ERR_ARG); (2 limit + 1)^3
 *   <= 2^27 cells, n_out <= 2^24, n_band <= 8, a list that holds one l plane, n_modes x n_freq within the work bound
 *   of csrc/size_guards.hpp (DS_ERR_UNSUP); DS_ERR_NOMEM, before anything is uploaded, when the device has not the
 *   memory free.                                                                                                   */
int ds_room_ism(ds_ctx* ctx, const double dim[3], const double src[3], const double rec[3], double sr, double c, int limit,
                const double* pw, int n_band, int64_t n_out, int64_t max_list_bytes, double* out);
int ds_room_modal_tf(ds_ctx* ctx, const double* omega_n, const double* eta, const double* weight, int64_t n_modes,
                     const double* omega2, int64_t n_freq, double* p);

/* ---- block-streaming FIR classes with device-resident state ------------------------------
 * One process_block of the reference's real-time classes (classes/fir_filter_realtime.py:75-335),
 * executed literally on buffers that stay on the device between calls; per call only the block
 * goes up and the filtered block comes back.
 * ds_fir_part_step_dev: FIRUniformPartitioned (:206-240) / FIRUniformPartitionedMultichannel
 *   (:296-335) for the channels [ch0, ch0 + n_call): shift the 2*bs input buffers, transform,
 *   store the spectra at slot `ind` of the delay line S[b][P][C], accumulate
 *   sum_p H[b][p][ch or 0] * S[b][(ind - p) mod P][ch], inverse transform, return the last bs
 *   samples.  inbuf [C][2 bs], block [n_call][bs], H [bs + 1][P][Cf] (Cf = 1: one impulse
 *   response for all channels, else Cf = C), out [n_call][bs].  The caller advances `ind`.
 * ds_fir_ols_step_dev: FIRFilterOverlapSave.process_block (:120-142) for ONE channel: buffer row
 *   [L] (L = next_fast_len(T + bs), any length), H [L / 2 + 1]; the inverse transform has the
 *   length numpy's irfft picks without an argument, 2 (L / 2) -- so for odd L the block is NOT
 *   the convolution, exactly as in the reference; the buffer is rolled by bs afterwards.     */
int ds_fir_part_step_dev(ds_ctx* ctx, float* inbuf_dev, const float* block_dev, int bs, int n_ch,
                         int ch0, int n_call, const ds_c32* h_dev, int n_part, int n_fir_ch,
                         ds_c32* delay_dev, int ind, float* out_dev);
int ds_fir_ols_step_dev(ds_ctx* ctx, float* buffer_row_dev, const float* block_dev, int bs,
                        int64_t total_length, const ds_c32* h_dev, float* out_dev);

/* ---- host marshalling (no device work): the reference hands (samples, channels) float64
 * C-order arrays (classes/signal.py:222-301) and expects the same back; the kernels take planar
 * float32.  Multi-threaded cast + transpose on the host (numpy's strided cast takes 0.2 s for the
 * 537 MB of the headline shape; this takes a fraction of it).  threads <= 0: min(16, cores).  */
int ds_host_planar_f32(const double* src, int64_t n_samples, int n_ch, float* dst, int64_t ld,
                       int threads);   /* dst[c*ld + n] = (float)src[n*n_ch + c] */
int ds_host_interleave_f64(const float* src, int64_t n_samples, int n_ch, int64_t ld, double* dst,
                           int threads); /* dst[n*n_ch + c] = (double)src[c*ld + n] */
int ds_host_widen_f64(const float* src, int64_t n, double* dst, int threads); /* dst[i] = (double)src[i] */

/* ---- FIR transfer functions: replaces scipy.signal.freqz(b, 1, worN=f, fs) in Filter.get_transfer_function
 * (classes/filter.py:862-900) and its per-filter loop in FilterBank.get_transfer_function
 * (classes/filterbank.py:615-655): out[k][i] = sum_n taps[k][n] exp(-2 pi i freqs_hz[i] n / fs_hz), float64.
 * taps [n_filt][n_taps] and out [n_filt][n_freq] are complex128 (interleaved doubles), host pointers.   */
int ds_fir_freqz(ds_ctx* ctx, const double* taps, int n_filt, int n_taps, const double* freqs_hz,
                 int n_freq, double fs_hz, double* out);

/* ---- variable-Q transform: transforms.vqt (transforms/transforms.py:812-923) in one call, float64 throughout
 * (csrc/kernels_vqt.hpp).  With P(x, up, down) scipy.signal.resample_poly's default filter for an integer ratio:
 * td_0 = P(x, 1, d), td_{o+1} = P(td_o, 1, 2); per octave o the same-mode convolution of td_o with each of the `bins`
 * complex kernels; every row back to the input rate by P(., 2^o, 1) (o > 0) and P(., d, 1), cut at n_samples.  Octave o's
 * kernel i is row n_oct * bins - 1 - (o * bins + i) of out (n_oct * bins, n_samples, n_ch) complex128: the reference's
 * flipped frequency axis.
 * x: x_on_device == 0: host (n_samples, n_ch) float64, ldx ignored; != 0: planar float32 on the device, channel c at
 * x + c * ldx, read where it lies and widened.  out: out_on_device == 0: a host array; != 0: a device buffer.
 * Host tables, built by the caller exactly as the reference builds them: kernel_len [bins], kernel_taps the kernels'
 * complex128 taps back to back; taps_dec = firwin(20 d + 1, 1 / d, kaiser 5.0) or the single tap 1.0 when d == 1;
 * taps_half = firwin(41, 1 / 2, ...); taps_up the interpolation filters back to back, 2^o * firwin(20 * 2^o + 1, 2^-o)
 * for o = 1 .. n_oct - 1, then d * firwin(20 d + 1, 1 / d) (the single tap 1.0 when d == 1).
 * Bounds (DS_ERR_UNSUP beyond, before anything is allocated): the result at most 2^34 bytes; d <= 48; n_oct <= 7 (the
 * first interpolation stage goes up to 2^6); kernels of at most 2048 taps; n_oct * bins and the channel groups of 4 at
 * most 65535.  DS_ERR_NOMEM, before anything is uploaded, when the device has not the memory free.
 * ds_resample_int: P alone on real host data, x (n, n_ch) float64 -> out (ceil(n * up / down), n_ch); one of up and down
 * is 1, the other at most 64 (48 for down); taps: up * firwin(20 r + 1, 1 / r, ...) with r = max(up, down), or the
 * single tap 1.0 when r == 1.                                                                                      */
int ds_vqt(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n_samples, int d, int n_oct,
           int bins, const int64_t* kernel_len, const double* kernel_taps, const double* taps_dec,
           const double* taps_half, const double* taps_up, void* out, int out_on_device);
int ds_resample_int(ds_ctx* ctx, const double* x, int64_t n, int n_ch, int up, int down, const double* taps,
                    double* out);

/* ---- rational-ratio resampling: standard.resample (standard/resampling.py:9-43), which is scipy.signal.resample_poly
 * with its default filter, in one launch, float64 arithmetic (csrc/kernels_resample.hpp).  up and down are coprime and
 * not both 1; r = max(up, down); taps: the host's up * firwin(20 r + 1, 1 / r, window=("kaiser", 5.0)), 20 r + 1 values.
 *     out[m] = sum_n x[n] taps[m down + 10 r - n up],   m < n_out = ceil(n up / down)
 * ds_resample_poly: x host (n, n_ch) float64 -> out host (n_out, n_ch) float64.
 * ds_resample_poly_dev: x planar float32 on the device, channel c at x + c * ldx, read where it lies and widened ->
 * y planar float32 on the device, channel c at y + c * ld_y (ld_y >= n_out), one rounding to float32 per value.
 * Bounds (DS_ERR_UNSUP beyond, before anything is allocated): r <= 640; max(n, n_out) * n_ch <= 2^31; n_ch <= 65535.
 * DS_ERR_NOMEM, before anything is uploaded, when the device has not the memory free.                             */
int ds_resample_poly(ds_ctx* ctx, const double* x, int64_t n, int n_ch, int up, int down, const double* taps,
                     double* out);
int ds_resample_poly_dev(ds_ctx* ctx, const float* x, int64_t ldx, int64_t n, int n_ch, int up, int down,
                         const double* taps, float* y, int64_t ld_y);

/* ---- audio effects: effects.Compressor, DigitalDelay, Chorus, Distortion, Tremolo (effects/effects.py) and the gate of
 * standard.activity_detector (standard/_standard_backend.py:324-379), float64 throughout (csrc/kernels_fx.hpp).
 * A stream is one channel of one band.  x_on_device == 0: x is a host (n, n_str) float64 array, y a host (n_out, n_str)
 * one, ldx and ld_y are ignored; != 0: both are planar float32 on the device, stream s at x + s * ldx and y + s * ld_y, and
 * the result stays there.  The small tables (coefficients, chorus indices, modulator) are host arrays the caller builds
 * as the reference does.  Bounds (DS_ERR_UNSUP beyond, before anything is allocated): 65535 streams, 2^28 padded samples
 * a stream, 2^30 in all, 8 curves, 64 voices.  DS_ERR_NOMEM, before anything is uploaded, when the memory is not free.
 * Compressor: par = { pre gain (linear), threshold dB, ratio, knee dB, attack coefficient, release coefficient, the
 *   floor of the squared sample, final gain (linear) }; with t = x pre_gain (divided by its stream's peak when
 *   `relative`), d = 10 log10(max(t^2, floor)), f = 10^((K(d) - d) / 20) for the knee curve K, the gain follows
 *   g <- c f + (1 - c) g from g = 1 with c the attack coefficient where f > g, else the release one; y = t g (times the
 *   peak again), times rms(x pre_gain) / rms(y) with `make_up`, times the final gain.
 * Detector: p = x^2 (x divided by its peak when `relative`); g[0] = 0, g[i] = c p[i] + (1 - c) g[i-1] with c = c_release
 *   where p[i-1] > 0, else 0; mask (n_str, n) bytes on the host: 10 log10(g) > threshold_db.
 * Delay: y[i] = x[i] + feedback sat(y[i - delay]) over n + padding samples (x zero beyond n), sat the identity
 *   (DS_FX_SAT_DIGITAL) or 0.5 atan(2 v) (DS_FX_SAT_ARCTAN); delay == 0 gives y = x + feedback sat(x) and needs padding 0;
 *   then the peak of x is restored.
 * Chorus: with td the samples followed by max_delay zeros, y[i] = (td[i] + sum_v td[i + m[i][v]]) mix + td[i] (1 - mix),
 *   a negative index counted from the end of td; then the peak of x is restored.  m: (n, voices) int32.
 * Distortion: y = gain * sum_k r_k, r_k = c_k peak(x) / peak(c_k), c_k = curve_k(x) mix_k; kinds DS_FX_CURVE_*,
 *   par (n_curves, 3) = linear level, linear offset, mix weight.  Curves whose weight is 0 are left out by the caller.
 * Tremolo: y[i] = x[i] mod[i].                                                                                        */
#define DS_FX_CURVE_ARCTAN 0
#define DS_FX_CURVE_HARD_CLIP 1
#define DS_FX_CURVE_SOFT_CLIP 2
#define DS_FX_CURVE_CLEAN 3
#define DS_FX_SAT_DIGITAL 0
#define DS_FX_SAT_ARCTAN 1
int ds_fx_compress(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, const double* par,
                   int downward, int relative, int make_up, void* y, int64_t ld_y);
int ds_fx_detect(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, double c_release,
                 double threshold_db, int relative, uint8_t* mask);
int ds_fx_delay(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, int64_t delay,
                int64_t padding, double feedback, int saturation, void* y, int64_t ld_y);
int ds_fx_chorus(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, const int32_t* m,
                 int voices, int64_t max_delay, double mix, void* y, int64_t ld_y);
int ds_fx_distort(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, int n_curves,
                  const int* kinds, const double* par, double gain, void* y, int64_t ld_y);
int ds_fx_tremolo(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, const double* mod,
                  void* y, int64_t ld_y);

/* ---- spectral subtraction: effects.SpectralSubtractor (effects/effects.py:138-550), float64 throughout
 * (csrc/kernels_specsub.hpp).  x, y, n_str, ldx, ld_y and x_on_device as for the effects above.  Every stream is padded
 * (virtually) by `window` zeros at both ends and cut into F = ceil((n + 2 window) / step) frames.  Per frame: the variance
 * of its samples gates it (10 log10(max(var, DBL_MIN)) < threshold_db), the frame times win_a is transformed, every bin's
 * magnitude becomes max(|X|^e - t, 0)^(1 / e) with the phase kept, the inverse transform is multiplied by win_s, and the
 * frames are overlap-added in ascending order and divided by the overlap-added win_s^2 (clipped from below at env_floor
 * when that is not negative) wherever it is above DBL_MIN; samples `window` .. `window` + n - 1 are kept and the peak of x
 * is restored (a stream subtracted to silence comes out as NaN).  DS_FX_SPECSUB_ADAPTIVE: t = factor N^e, where the
 * amplitude estimate N starts at 0 and becomes N forgetting + |X| (1 - forgetting) at every gated frame, that frame's
 * own bins included; `table` is not read.  DS_FX_SPECSUB_STATIC: t = factor table[stream][bin], table a host
 * (n_str, window / 2 + 1) array, and neither the gate nor `forgetting` has an effect.  win_a, win_s: host [window].
 * window: a power of two, 4 .. 16384; 1 <= step <= window.  DS_ERR_UNSUP beyond 16384, a frame workspace
 * 8 (window + 2) F n_str above 2^32 bytes, n n_str ceil(window / step) above 2^29, or the effects' bounds, before
 * anything is allocated; DS_ERR_NOMEM, before anything is uploaded, when the memory is not free.                       */
#define DS_FX_SPECSUB_ADAPTIVE 0
#define DS_FX_SPECSUB_STATIC 1
int ds_fx_specsub(ds_ctx* ctx, const void* x, int x_on_device, int n_str, int64_t ldx, int64_t n, const double* win_a,
                  const double* win_s, int window, int step, int mode, double threshold_db, double forgetting,
                  double factor, double exponent, const double* table, double env_floor, void* y, int64_t ld_y);

/* ---- levels and loudness: normalize, rms, crest_factor, fade, apply_gain (standard/gain_and_level.py:12-118, 169-200,
 * 284-401 with helpers/gain_and_level.py:7-155), detrend and envelope (standard/other.py:182-284,
 * standard/_standard_backend.py:382-405) and the block energies of lufs_integrated (standard/gain_and_level.py:203-281),
 * float64 throughout, every sum in a fixed order (csrc/kernels_level.hpp).
 * x_on_device == 0: x is a host (n, n_ch) float64 array and ldx is ignored; != 0: planar float32 on the device, channel c
 * at x + c * ldx, read where it lies.  A polynomial trend of `order` 0 .. 8 (order < n) is the least-squares one in the
 * discrete Chebyshev polynomials orthonormal on 0 .. n - 1; basis: host [18] = (n - 1) / 2, 1 / sqrt(n), a_0 .. a_7,
 * b_0 .. b_7 of P_{k+1} = a_k t P_k - b_k P_{k-1}, t = i - (n - 1) / 2, read up to the order (the caller forms them in
 * long double).  Bounds (DS_ERR_UNSUP beyond, before anything is allocated): 65535 channels, 2^31 - 1 samples a channel,
 * 2^33 in all; DS_ERR_NOMEM, before anything is uploaded, when the memory is not free.
 * ds_level_project: out (n_ch, 10) = sum_i x[i] P_k(i) for k = 0 .. 8 (0 past the order), max |x|.
 * ds_level_stats: out (n_ch, 3) = sum (x - p)^2 term by term, max |x - p|, max |x|, p the channel's trend; `common`
 *   (order 0): the mean of all channels together is removed instead (numpy's std of the flattened array).
 * ds_level_apply: y[i] = (x[i] - p_c(i)) g_c fade[i] fade[n - 1 - i], one rounding per factor in this order, an absent
 *   factor skipped: order < 0 no trend; g the host's gain[n_ch] or NULL, or with norm_mode DS_LEVEL_NORM_* the device's
 *   norm_factor / max |x| or norm_factor / sqrt(mean (x - mean)^2) of each channel or of all; fade the host's
 *   fade[l_fade], 1 <= l_fade <= n, applied to the first l_fade samples (at_start) and mirrored to the last (at_end).
 *   y as x: host (n, n_ch) float64, or planar float32 rows of pitch ld_y on the device, where the result stays.
 * ds_moving_rms: out (n, n_ch) = sqrt(max(0, sum of the squares of x - line over the last w samples / w)), samples before
 *   the first counted as zero, w >= 1 (w may exceed n); basis of order 1.  The mean square is rebuilt every 1024 outputs:
 *   its error does not grow along the signal.  n_ch * n * (2 + min(w, n) / 1024) at most 1e12.
 * ds_loudness_blocks: the cascade sos (n_sec, 6), 1 <= n_sec <= 32, on the float64 section runner of ds_iir_sos from rest, then
 *   z (n_blocks, n_ch) = mean of the tg squares from sample b * step on; n > tg, n_blocks == ceil((n - tg) / step).
 * ds_envelope_analytic: out (n, n_ch) = |hilbert(x - line)| on the transform of ds_hilbert and within its length bounds;
 *   basis of order 1.                                                                                                */
#define DS_LEVEL_NORM_NONE 0
#define DS_LEVEL_NORM_PEAK_EACH 1
#define DS_LEVEL_NORM_PEAK_ALL 2
#define DS_LEVEL_NORM_RMS_EACH 3
#define DS_LEVEL_NORM_RMS_ALL 4
int ds_level_project(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n, int order,
                     const double* basis, double* out);
int ds_level_stats(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n, int order,
                   const double* basis, int common, double* out);
int ds_level_apply(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n, int order,
                   const double* basis, int norm_mode, double norm_factor, const double* gain, const double* fade,
                   int64_t l_fade, int at_start, int at_end, void* y, int64_t ld_y);
int ds_moving_rms(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n, const double* basis,
                  int64_t w, double* out);
int ds_loudness_blocks(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n, const double* sos,
                       int n_sec, int64_t tg, int64_t step, int64_t n_blocks, double* z);
int ds_envelope_analytic(ds_ctx* ctx, const void* x, int x_on_device, int n_ch, int64_t ldx, int64_t n,
                         const double* basis, double* out);

/* ---- multi-GPU: RCCL over xGMI, one process per GPU -----------------------
 * The hot path has no exchange step: the only collectives are the
 * broadcast of a shared input (sweep / taps / inverse spectrum) and the gather of sharded
 * results.  Rank 0 creates the id, the host exchange (dsptoolbox_amd/rendezvous.py: a TCP
 * star; or a file, MPI, a torch.distributed store ...) hands the 128 bytes to every rank.
 * ds_allgather: rank r's bytes_per_rank bytes at send_dev land at recv_dev + r * bytes_per_rank
 * on every rank (ncclAllGather on the context's stream; send may alias its own slot).  */
int ds_comm_unique_id(char id_out[128]);
int ds_comm_init(ds_ctx* ctx, int n_ranks, int rank, const char id[128]);
/* ranks of that communicator as RCCL counts them (ncclCommCount): what a multi-GPU bench line reports */
int ds_comm_count(ds_ctx* ctx, int* n_ranks);
int ds_bcast(ds_ctx* ctx, void* buf_dev, size_t bytes, int root);
int ds_allgather(ds_ctx* ctx, const void* send_dev, void* recv_dev, size_t bytes_per_rank);
int ds_comm_destroy(ds_ctx* ctx);

/* ---- measurement: device-to-device copy bandwidth of THIS GPU (a 16-byte-per-lane streaming
 * copy kernel over `bytes` bytes, `reps` timed launches after one warm-up; GB/s counts read +
 * written bytes) -- the measured denominator bench.py reports next to the nominal 8 TB/s
 * (SURVEY.md section 8(d)).                                                                  */
int ds_measure_copy(ds_ctx* ctx, size_t bytes, int reps, double* gb_per_s);
/* free / total device memory of the context's GPU (hipMemGetInfo), for leak checks */
int ds_mem_info(ds_ctx* ctx, size_t* free_bytes, size_t* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DSPTOOLBOX_AMD_H */
