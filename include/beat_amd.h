/*
 * beat_amd.h -- C ABI of libbeat_amd.so: the MI355X (gfx950) forward-model +
 * likelihood engine for BEAT's SMC/PT inner loop.
 *
 * This is the drop-in boundary (DESIGN.md "Boundary"): plain pointers and sizes, no
 * torch / numpy / Python types.  Each entry point names the reference interface it
 * replaces (file:line under hvasbath/beat v2.0.5).  INTEGRATION.md shows the ctypes
 * stubs a BEAT maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success or a negative BEATAMD_E* code;
 *    beatamd_last_error() returns the thread-local message of the last failure.
 *  - all arrays are C-contiguous IEEE float64 unless stated; indices are int32.
 *  - array arguments may be HOST pointers (numpy) or DEVICE pointers (HBM, e.g. a torch
 *    tensor's data_ptr()); the library detects which (hipPointerGetAttributes) and
 *    stages host buffers through context-owned HBM scratch.  With device pointers no
 *    copy is made and the call is asynchronous on the context stream; with host
 *    pointers the call returns after the results are back in host memory.
 *  - "C" is the number of Markov chains in the batch: chains are the batch dimension
 *    of every kernel (the reference evaluates one chain per call).
 *  - one beatamd_ctx per (process, GPU); a context is not thread-safe.
 */
#ifndef BEAT_AMD_H
#define BEAT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEATAMD_OK 0
#define BEATAMD_EINVAL (-1)   /* bad argument (reference: AttributeError / ValueError)   */
#define BEATAMD_EHIP (-2)     /* HIP runtime failure                                       */
#define BEATAMD_EINDEX (-3)   /* index outside the GF library (reference: numpy IndexError) */
#define BEATAMD_ENOMEM (-4)
#define BEATAMD_ENAN (-5)     /* non-finite likelihood at stage 0 (metropolis.py:279-284)  */
#define BEATAMD_ENOTPSD (-6)  /* covariance not positive definite (numpy.linalg.LinAlgError) */
#define BEATAMD_EOUTSIDE (-8) /* a line leaves the density grid (plotting/common.py:733-739: TypeError) */
#define BEATAMD_EBADCOV (-7)  /* weighted sample covariance of the population contains Inf/NaN
                               * (reference: ValueError of SMC.calc_covariance, sampler/smc.py:167-186) */

/* ABI revision: bumped whenever an entry point changes its signature or an error code is added
 * (1.1: beatamd_weights_update gained kind/count in round 2; BEATAMD_EBADCOV).  beat_amd/_lib.py
 * refuses a library whose revision differs from the header it was written against.  BEATAMD_EOUTSIDE came with
 * beatamd_trace_density_update inside revision 120: only that entry returns it. */
#define BEATAMD_VERSION 120

#define BEATAMD_NEAREST_NEIGHBOR 0 /* interpolation="nearest_neighbor" */
#define BEATAMD_MULTILINEAR 1      /* interpolation="multilinear"      */

#define BEATAMD_W_SCALAR 0 /* W_i = w_i * I   (chol_inverse of sigma^2 I)            */
#define BEATAMD_W_DENSE 1  /* W_i dense (M,M) row-major, upper-triangular content    */

#define BEATAMD_DOMAIN_TIME 0     /* WaveformFitConfig.domain = "time" (heart.py:526)                  */
#define BEATAMD_DOMAIN_SPECTRUM 1 /* "spectrum": amplitude spectra, beatamd_ffi_model_add_wavemap_spectrum */

typedef struct beatamd_ctx beatamd_ctx;

const char *beatamd_last_error(void);
int beatamd_version(void);

/* ---------------------------------------------------------------- context --------- */
int beatamd_ctx_create(int device, beatamd_ctx **out);
int beatamd_ctx_destroy(beatamd_ctx *ctx);
/* launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).
 * NULL is a valid handle: the HIP null (legacy default) stream, which is what torch uses
 * unless a side stream is current.  beatamd_ctx_use_own_stream goes back to the context's
 * private non-blocking stream. */
int beatamd_ctx_set_stream(beatamd_ctx *ctx, void *hip_stream);
int beatamd_ctx_use_own_stream(beatamd_ctx *ctx);
int beatamd_ctx_synchronize(beatamd_ctx *ctx);
/* The A/B and test knobs of the stacking path (environment variables BEATAMD_GF_*, BEATAMD_GS_*, BEATAMD_GC_*,
 * BEATAMD_GR_*, BEATAMD_WS_MAP, BEATAMD_SWEEP_V1; defaults = the shipped path) are read ONCE, when the context is
 * created.  This call reads them again.  A context created while BEATAMD_KNOBS_LIVE=1 is in the environment re-reads
 * them at every stacking call (test suites and A/B tools that compare kernels inside one process). */
int beatamd_ctx_reload_knobs(beatamd_ctx *ctx);
/* Device-resident step counter of the proposal generator.  With a counter set (uint32 in device
 * memory, NULL to unset) beatamd_proposal_draw / _univariate take the Philox step from it instead
 * of their `step` argument and add one to it afterwards: a Metropolis step captured in a HIP graph
 * (nothing in it synchronises with the host) then replays with fresh, reproducible draws --
 * the launch-bound geometry-mode problems run from a graph (beat_amd/sampler/metropolis.py). */
int beatamd_ctx_set_step_counter(beatamd_ctx *ctx, uint32_t *device_counter);
/* per-kernel HIP-event timing on the launch stream (bench.py roofline leg).
 * kernel names: "sweep", "tables", "gfstack", "quadform", "geostack", "finish", "astep" */
int beatamd_ctx_enable_timing(beatamd_ctx *ctx, int on);
int beatamd_ctx_kernel_time(beatamd_ctx *ctx, const char *kernel, double *total_ms,
                            int64_t *launches);
int beatamd_ctx_reset_timing(beatamd_ctx *ctx);
/* name and template arguments of the stacking kernel the most recent stack_all / logp / astep call
 * launched, e.g. "k_gfstack_dma<8,1,1,64,1>" (wavefronts per workgroup, rows per patch, epilogue,
 * samples per tile, ds_read_b64 layout) or "k_gfstack<0,1,1,2,0>" (streaming form). */
int beatamd_ctx_last_kernel(beatamd_ctx *ctx, char *buf, int64_t buflen);
/* chain-shared stacking kernels: distinct library rows per (chain group, target, patch) of the most
 * recent launch -- mean, maximum, and the bytes of library rows staged from HBM (sum x N x 8).
 * chains_per_group = 0 / row_bytes = 0 when the streaming kernel ran.  Synchronises. */
int beatamd_ctx_gf_group_stats(beatamd_ctx *ctx, int64_t *chains_per_group, double *mean_rows,
                               int64_t *max_rows, int64_t *row_bytes);
/* which stacking kernel the selection chose for the most recent launch and why, in words (chains per group, LDS row
 * slots, whether patches are staged in several row passes), and -- when asked for (non-NULL; synchronises) -- the row
 * passes per (chain group, target, patch) of that launch: 1 everywhere unless a patch touched more distinct library
 * rows than an LDS row buffer holds.  No reference counterpart: the reference gathers one chain's rows by fancy
 * indexing (beat/ffi/base.py:651-704); this reports how the batch shares them. */
int beatamd_ctx_gf_plan(beatamd_ctx *ctx, char *buf, int64_t buflen, double *mean_passes, int64_t *max_passes);
/* the chain-group size of the lane <-> chain stacking kernels is MEASURED on the first call of a problem shape (every
 * candidate launched twice on the real inputs, the fastest kept; from 1024 chains on only 512 / 256 are candidates):
 * this returns the most recent measurement in words ("group size for 4096 chains (...): 512: 35.8 ms, 256: 61.2 ms ->
 * 512"), empty before the first one.  BEATAMD_VERBOSE=1 prints the same line to stderr when it happens.  No reference
 * counterpart (the reference has no batch; beat/ffi/base.py:607-709 stacks one chain). */
int beatamd_ctx_gf_tune_log(beatamd_ctx *ctx, char *buf, int64_t buflen);
/* Libraries of short traces (nsamples <= 256: the usual 60 s at 2 Hz of an FFI set-up) are stacked in R patch
 * RANGES -- the same memory viewed as [T*R, P/R, D, S, N], the ranges' partial synthetics summed in range order -- so that
 * T * ceil(N/64) walks of P serial steps become R times as many, R times shorter ones for the device's compute units.
 * This is the rule (a pure function; num_cu <= 0: 256): R = the divisor of P with >= 32 patches per range that minimises
 * ceil(walks * R / num_cu) * (P / R + 5); 1 = the library as it is.  What a call did is in beatamd_ctx_gf_plan.  No reference
 * counterpart (beat/ffi/base.py:607-709 stacks one chain on one core). */
int32_t beatamd_gf_patch_ranges(int64_t ntargets, int64_t npatches, int64_t nsamples, int32_t num_cu);
/* The rupture onset times the model's forward pass starts from: times[C, npatches] = fast sweep of every subfault from
 * the hypocentre and the velocities in Q plus the subfault's nucleation time (seismic.py:1253-1272), as
 * beatamd_ffi_logp_batch computes them.  chain_bad[C] (nullable): 1 for a chain whose hypocentre index lies outside the
 * patch grid; the call then fills both arrays and returns BEATAMD_EINVAL. */
int beatamd_ffi_start_times_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *times,
                                  int32_t *chain_bad);
/* ---- moment, moment magnitude and moment-rate functions of a batch of draws (momentrate.hip) ----
 * Common arguments: Q [C, nparams]; moment_per_slip [npatches] = the moment of every patch at unit slip (mu * area from
 * the store: pyrocko's RectangularSource.get_moment is linear in the slip); comp_off [ncomp] (host or device, <= 4) =
 * offsets in q of the slip variables the total slip is formed from, NULL: the layout's own (get_total_slip with
 * components=None); start_times [C, npatches] with chain_bad [C] (nullable) = onsets the caller already holds, as
 * beatamd_ffi_start_times_batch returns them, NULL: the model's own sweep is run.  All arithmetic is FP64, contraction off.
 *
 * replaces: FaultGeometry.get_moment / get_magnitude / get_total_slip / get_subfault_patch_moments
 *           beat/ffi/fault.py:284-359 (per draw, a Python loop over the patches; `beat summarize --calc_derived`
 *           through get_derived_parameters, fault.py:945-954)
 *   M0[c] = sum_p k_p * sqrt(sum_comp s_{c,p,comp}^2), the patches added in patch order from 0.0; a patch of zero slip
 *   contributes exactly 0 (fault.py:309-312).  Mw[c] = log10(M0 * 1e7) / 1.5 - 10.7, 0 where M0 == 0 (fault.py:338-341).
 *   DEVIATIONS: the reference's num.array(moments).sum() is numpy's pairwise sum (differs within npatches * 2^-53
 *   relative); the magnitude formula is pyrocko's moment_to_magnitude AS RECALLED -- pyrocko was not available to check
 *   it against: UNVERIFIED. */
int beatamd_ffi_magnitudes_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, const double *moment_per_slip,
                                 const int64_t *comp_off, int32_t ncomp, double *M0, double *Mw);
/* replaces: the time axes of get_subfault_moment_rate_function / get_moment_rate_function   beat/ffi/fault.py:413-420, 461-465
 *   spans [C, nsubfaults + 1, 2] (int64) = (first, count) per subfault, the total in row nsubfaults:
 *       first = floor(min_p start / deltat),  count = ceil((max_p start + max_allP duration) / deltat) + 1 - first
 *   (the largest duration is the whole fault's, as point["durations"].max()); the total spans all subfaults.
 *   DEVIATION: integer index grids instead of num.arange on floats -- a time is index * deltat; the lengths agree wherever
 *   the reference's float steps are exact (deltat a power of two).  A draw flagged in chain_bad (hypocentre outside the
 *   patch grid) gets count = 0 in every row and the call returns BEATAMD_EINVAL after filling the array; so does a draw
 *   with an onset or duration that is not finite, a negative duration or an index beyond 2^40 (the reference fails in
 *   arange there). */
int beatamd_ffi_moment_rate_spans_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q,
                                        const double *start_times, const int32_t *chain_bad, double deltat, int64_t *spans);
/* replaces: get_subfault_patch_stfs / get_subfault_moment_rate_function / get_moment_rate_function
 *           beat/ffi/fault.py:361-474 (per draw: a Python loop over the patches around pyrocko's stf.discretize_t)
 *   rates [C, nsubfaults + 1, NT] on the index grid [kbase, kbase + NT) (sample j at (kbase + j) * deltat): rows
 *   0 .. nsubfaults - 1 the subfaults, row nsubfaults their sum in subfault order (fault.py:466-472); zero outside a
 *   draw's span; a moment per sample, not divided by deltat, as in the reference.  Per patch, in patch order, with
 *   t0 = start, t1 = start + duration (anchor -1, beat/ffi/base.py:1013) and m = k_p * sqrt(sum_comp s^2) (fault.py:412
 *   passes uparr and uperp):
 *       k0 = round(t0 / deltat), k1 = round(t1 / deltat) (half to even), nt = k1 - k0 + 1
 *       nt == 1: a = [1];  else  e_i = max(t0, min(t1, k0 deltat + (i - 0.5) deltat)), i = 0 .. nt,
 *       F_i = -cos((e_i - t0) (pi / duration)), a_i = F_{i+1} - F_i, a_i /= S;   rate[k0 - kbase + i] += a_i * m
 *   S adds the a_i in one fixed order: 64 strided partial sums (i = l, l + 64, ...), folded 32/16/8/4/2/1.  Rows are
 *   independent: a batch cut into calls or permuted gives the same bits.  stf: BEATAMD_STF_HALF_SINUSOID; any other value
 *   is BEATAMD_EINVAL (Boxcar and Triangular are not built).  spans (nullable): as beatamd_ffi_moment_rate_spans_batch.
 *   NT is limited to 20224 (the row lives in LDS): BEATAMD_EINVAL above.  A draw whose total span does not lie within the
 *   grid gets NaN rows and the call returns BEATAMD_EINVAL after filling the arrays; so does a draw with count = 0.
 *   DEVIATIONS: integer index grids (above); the reference's num.sum(amplitudes) is numpy's pairwise sum; the
 *   discretisation is pyrocko's HalfSinusoidSTF.discretize_t with exponent = 1 (BEAT's default stf_type) AS RECALLED --
 *   pyrocko was not available to check it against: UNVERIFIED. */
#define BEATAMD_STF_HALF_SINUSOID 0
int beatamd_ffi_moment_rates_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, const double *moment_per_slip,
                                   const int64_t *comp_off, int32_t ncomp, const double *start_times, const int32_t *chain_bad,
                                   double deltat, int32_t stf, int64_t kbase, int64_t NT, double *rates, int64_t *spans);
/* The LDS bytes a workgroup of the rupture-time sweep asks for when the largest subfault of a batch has ncells patches,
 * and through waves (nullable) how many grids share that workgroup (4 or 1): a pure function, the rule of the launch
 * (four grids per workgroup while they fit 64 KiB together, one above; at most 160 KiB).  -1: ncells is not in 1..6400,
 * the limit of beatamd_fast_sweep_batch.  No reference counterpart (fast_sweep_ext.c solves one grid on the host). */
int32_t beatamd_fast_sweep_lds(int32_t ncells, int32_t *waves);
/* The target count the rule above sees for a library (default 0: its own T).  R sets the order in which a target's patches
 * are summed, so a rank's block of a library sharded by target (beat_amd/models/sharded.py) is given the whole wavemap's
 * target count: every rank then picks the R of the replicated library, and the likelihoods stay bitwise those of the
 * replicated model.  ntargets = 0 or >= the library's T.  No reference counterpart (the reference does not shard). */
int beatamd_seis_gflib_set_split_targets(beatamd_ctx *ctx, int32_t lib_id, int64_t ntargets);

/* how a batch of C chains is cut into its chain groups (scheduling only; results never depend on it): recursive
 * bisection of the batch along the key in which a part's chains spread wider -- the fused model path hands the hypocentre
 * (strike, dip) of every chain, so that a group covers a compact piece of the fault and stages fewer distinct library rows.
 *   key0 / key1 [C] (device)   members [ceil(C / chains_per_group) * chains_per_group] (host): members[g * cpg + i] =
 *   i-th chain of group g, 0xffffffff behind the last chain.  Batches beyond 8192 chains (or 64 groups) are cut chunk by chunk: chunks of min(8192 / chains_per_group, 64) whole groups as the chains come, each bisected on its own (chains_per_group <= 8192).
 * No reference counterpart (the reference evaluates one chain per process, beat/sampler/base.py:428-595). */
int beatamd_ctx_gf_chain_groups(beatamd_ctx *ctx, int64_t C, const double *key0, const double *key1,
                                int64_t chains_per_group, uint32_t *members);

/* ---------------------------------------------------------------- fast sweep -------
 * replaces: fast_sweep_ext.fast_sweep(slowness, patch_size, h_strk, h_dip, num_strk,
 *           num_dip)                       beat/fast_sweeping/fast_sweep_ext.c:120-245
 *           pytensorf.Sweeper.perform      beat/pytensorf.py:443-500
 * Batched over chains.  Same argument slots as the C extension: rows i in
 * [0,num_strk), columns j in [0,num_dip), flat index i*num_dip + j (BEAT passes
 * dip in the "strk" slots, pytensorf.py:473-482).
 *   slowness [C, num_strk*num_dip]   h_strk/h_dip [C] int32   out [C, num_strk*num_dip]
 * A hypocentre index outside the grid is BEATAMD_EINVAL (the reference writes out of
 * bounds). */
int beatamd_fast_sweep_batch(beatamd_ctx *ctx, const double *slowness, double patch_size,
                             const int32_t *h_strk, const int32_t *h_dip, int32_t num_strk,
                             int32_t num_dip, int64_t C, double *out);

/* ---------------------------------------------------------------- GF libraries -----
 * replaces: SeismicGFLibrary (5-D float64 array (ntargets, npatches, ndurations,
 *           nstarttimes, nsamples) + index maps)          beat/ffi/base.py:320-709
 *           init_optimization() / parallel.memshare: one HBM-resident copy per GPU
 *                                              beat/ffi/base.py:387-404, parallel.py:285-439 */
int beatamd_seis_gflib_create(beatamd_ctx *ctx, int64_t ntargets, int64_t npatches,
                              int64_t ndurations, int64_t nstarttimes, int64_t nsamples,
                              double starttime_min, double starttime_sampling,
                              double duration_min, double duration_sampling, int32_t *lib_id);
/* copy `count` doubles (host or device source) to element offset `offset` of the library */
int beatamd_seis_gflib_upload(beatamd_ctx *ctx, int32_t lib_id, const double *src,
                              int64_t offset, int64_t count);
/* use a caller-owned device allocation as the library storage (no copy) */
int beatamd_seis_gflib_adopt(beatamd_ctx *ctx, int32_t lib_id, double *device_ptr);
/* float storage (SURVEY 8(f) row 2 "optional fp32 layout"; the reference keeps its libraries in
 * float64, beat/ffi/base.py:381-385 tconfig.floatX aside).  beatamd_seis_gflib_round_to_f32 ROUNDS THE
 * LIBRARY IN PLACE -- the float64 storage (also a caller-owned adopted allocation) is overwritten with
 * (double)(float)value, irreversibly, values change by up to 6e-8 relative -- and keeps a float copy of
 * the same values in HBM, so that every kernel, whichever copy it reads, works on ONE library.
 * Accumulation, weights and likelihoods stay float64.  Never called by the library itself.
 * beatamd_ffi_model_set_f32 lets a wavemap of a model read the float copies where a kernel exists for
 * them (on = 0: the float64 kernels on the same rounded values; it does NOT restore anything).  An upload
 * into the library or an in-place whitening of its rows (beatamd_whiten_rows) drops the float copy and
 * takes every wavemap off it: the copies would no longer agree. */
int beatamd_seis_gflib_round_to_f32(beatamd_ctx *ctx, int32_t lib_id);
int beatamd_ffi_model_set_f32(beatamd_ctx *ctx, int32_t model_id, int32_t wavemap_index, int32_t on);
int beatamd_seis_gflib_device_ptr(beatamd_ctx *ctx, int32_t lib_id, double **device_ptr);
int beatamd_seis_gflib_destroy(beatamd_ctx *ctx, int32_t lib_id);

/* replaces: SeismicGFLibrary.stack_all(durations, starttimes, slips, targetidxs,
 *           patchidxs, interpolation)                      beat/ffi/base.py:607-709
 *           (incl. starttimes2idxs :486-521, durations2idxs :535-568)
 *   durations [C,P]  starttimes [C,T,P]  slips [C,P]  ->  out [C,T,N]
 * An index outside the library is BEATAMD_EINDEX (numpy IndexError); negative indices
 * wrap like numpy. */
int beatamd_seis_stack_all_batch(beatamd_ctx *ctx, int32_t lib_id, int64_t C,
                                 const double *durations, const double *starttimes,
                                 const double *slips, int32_t interpolation, double *out);

/* replaces: GeodeticGFLibrary.stack_all(slips) = G.T.dot(slips)  beat/ffi/base.py:292-305
 *   G [P,Nobs] (uploaded once)   slips [C,P]  ->  out [C,Nobs]; accumulate!=0 adds */
int beatamd_geo_gflib_create(beatamd_ctx *ctx, int64_t npatches, int64_t nobs, const double *G,
                             int32_t *lib_id);
int beatamd_geo_gflib_destroy(beatamd_ctx *ctx, int32_t lib_id);
int beatamd_geo_stack_all_batch(beatamd_ctx *ctx, int32_t lib_id, int64_t C,
                                const double *slips, int32_t accumulate, double *out);

/* ---------------------------------------------------------------- velocity-model prediction covariance -------
 * replaces: the crust-variant loop of GeodeticDistributerComposite.update_weights
 *                                                        beat/models/geodetic.py:1161-1176
 *           (mu_k = sum over slip variables of gfs[key(crust_ind, var)].stack_all(point[var]), ffi/base.py:292-305)
 * An ensemble names K * nvar existing beatamd_geo_gflib libraries, variant-major (lib_ids[k * nvar + v]; host or
 * device array): the libraries of K crust-model variants for nvar slip variables.  All must share (P, Nobs), else
 * BEATAMD_EINVAL.  The ensemble owns none of them; stacking an ensemble one of whose libraries was destroyed or
 * re-created is BEATAMD_EINVAL.
 *   stack: slips [nvar*P] (one point) -> X [K, Nobs].  Per (variant, observation) the operation sequence of
 *   beatamd_geo_stack_all_batch / the model's geodetic composite (variables ascending, patches ascending, one fma per
 *   term from 0): the row of the variant that is a model's own library is that model's mu bit for bit. */
int beatamd_geo_ensemble_create(beatamd_ctx *ctx, const int32_t *lib_ids, int64_t K, int64_t nvar, int32_t *ens_id);
int beatamd_geo_ensemble_destroy(beatamd_ctx *ctx, int32_t ens_id);
int beatamd_geo_ensemble_stack(beatamd_ctx *ctx, int32_t ens_id, const double *slips, double *X);
/* replaces: cov_pv = num.cov(crust_synths[i], rowvar=0) per dataset and its addition to the other covariance terms
 *                                                        beat/models/geodetic.py:1185-1190, beat/heart.py:158-164
 *   X [K, Nobs] (the ensemble's synthetics), nd datasets of sizes[i] columns each (their sum is Nobs), dataset i at
 *   column offset o_i = sizes[0] + ... + sizes[i-1]:
 *       mean_j = (sum_k X[k,j]) / K;   D[k,j] = X[k,j] - mean_j;
 *       out[i][a,b] = base[i][a,b] + (sum_k D[k,o_i+a] * D[k,o_i+b]) / (K - 1)
 *   every sum over k ascending from 0, plain products and sums, true divisions: a numpy restatement gives the same
 *   bits, and out[i] is exactly symmetric where base[i] is.  base (or an entry of it) NULL: zeros.  base / out are
 *   host arrays of nd pointers; the matrices [sizes[i], sizes[i]] they point to, X and sizes may live on either side.
 *   K < 2 is BEATAMD_EINVAL (numpy divides by zero).  DEVIATION: the reference passes cov_pv through
 *   utility.ensure_cov_psd (utility.py:1034-1056) before adding it; here the raw sample covariance is added and the
 *   factorisation of the total (beatamd_chol_inverse_batch_flags) decides -- beat_amd.covariance repairs on the host
 *   what that flags. */
int beatamd_pred_covariance_batch(beatamd_ctx *ctx, int64_t K, int64_t Nobs, const double *X, int64_t nd,
                                  const int64_t *sizes, const double *const *base, double *const *out);

/* ---------------------------------------------------------------- likelihood -------
 * replaces: multivariate_normal_chol(datasets, weights, hyperparams, residuals)
 *                                              beat/models/distributions.py:72-140
 * A "weight set" holds what the reference keeps in pytensor shared variables per
 * dataset: W_i = Covariance.chol_inverse (heart.py:211-237), slog_pdet_i
 * (heart.py:239-253) and M_i = nsamples.  All datasets of a set share M.
 *   kind SCALAR: weights [nd]      kind DENSE: weights [nd, M, M]
 * update = SeismicComposite.update_weights (seismic.py:1509-1534): same call again. */
int beatamd_weights_create(beatamd_ctx *ctx, int32_t kind, int64_t ndatasets, int64_t M,
                           const double *weights, const double *slog_pdet, int32_t *wset_id);
/* kind and count (number of doubles in `weights`) are validated against the set: a wavemap whose
 * library was pre-whitened holds scalar weights and rejects a dense update (re-whiten instead). */
int beatamd_weights_update(beatamd_ctx *ctx, int32_t wset_id, int32_t kind, int64_t count,
                           const double *weights, const double *slog_pdet);
int beatamd_weights_destroy(beatamd_ctx *ctx, int32_t wset_id);
/* BANDED whitening operators.  The reference's "exponential" noise structure (beat/covariance.py:24-51:
 * C_ij = exp(-|i-j| dt / t0), a Markov kernel) has a BIDIAGONAL W = chol(inv(C)).T -- what numpy's inv + cholesky leave
 * outside the band is rounding residue (~2e-15 of the largest entry).  A DENSE weight set whose matrices are all
 * upper-triangular with no entry further than 16 columns right of the diagonal above 2^-40 of its matrix's largest entry is
 * therefore evaluated on its band (two products per sample for the bidiagonal case instead of a matrix row; the dropped
 * entries change a whitened sample by < M * 2^-40 of its largest term, far inside the 1e-6 tolerance of the path).
 * *band = the half bandwidth in use, -1 when the dense kernel is used.  BEATAMD_QF_BAND=0 (environment) keeps the dense
 * kernel for every set. */
int beatamd_weights_band(beatamd_ctx *ctx, int32_t wset_id, int64_t *band);
/* the same with what the banded evaluation leaves out: max_dropped_rel = the largest |entry| beyond the band relative to the
 * largest |entry| of its own row (<= 2^-40 by construction; 0 for an exactly banded operator; rounding residue of
 * inv + cholesky, ~2e-15, for the reference's "exponential" structure, beat/covariance.py:24-51 through heart.py:201-253).
 * A caller logs it once per weights_create / weights_update (beat_amd.models.problem does); BEATAMD_VERBOSE=1 prints the
 * detection to stderr.  band = -1: evaluated by the dense kernel. */
int beatamd_weights_band_info(beatamd_ctx *ctx, int32_t wset_id, int64_t *band, double *max_dropped_rel);
/*   residuals [C, nd, M]   hp [C, nd] (hyperparameter already resolved per dataset,
 *   distributions.py:117-126)   ->   logpts [C, nd]                                  */
int beatamd_mvn_chol_logp_batch(beatamd_ctx *ctx, int32_t wset_id, int64_t C,
                                const double *residuals, const double *hp, double *logpts);

/* replaces: LaplacianDistributerComposite.get_formula / _eval_prior
 *                                              beat/models/laplacian.py:88-139
 *   L [P,P]  slips [C, nvar, P]  hp [C]  ->  out [C]  (sum over slip variables)      */
int beatamd_laplacian_create(beatamd_ctx *ctx, int64_t npatches, const double *L,
                             double logdet, int32_t *lap_id);
int beatamd_laplacian_destroy(beatamd_ctx *ctx, int32_t lap_id);
int beatamd_laplacian_logp_batch(beatamd_ctx *ctx, int32_t lap_id, int64_t C, int64_t nvar,
                                 const double *slips, const double *hp, double *out);

/* ---------------------------------------------------------------- fused FFI model ---
 * replaces: the compiled logp_forw_func(q) of a DistributionOptimizer (FFI) problem:
 *           sampler/base.py:598-615 logp_forw; graph built by
 *           SeismicDistributerComposite.get_formula   beat/models/seismic.py:1210-1349
 *           GeodeticDistributerComposite.get_formula  beat/models/geodetic.py:1030-1084
 *           LaplacianDistributerComposite.get_formula beat/models/laplacian.py:98-139
 *           Problem.built_model (like = sum)          beat/models/problems.py:212-248
 * Q [C, nparams] -> LL [C, nllk]; nllk = sum(seismic datasets) + sum(geodetic
 * datasets) + (laplacian ? 1 : 0) + 1, ordered seis_like.., geo_like.., laplacian_like,
 * like  (SURVEY Appendix C "Outputs").
 * Offsets are positions in the flat parameter vector q (DictToArrayBijection order,
 * taken from the host model); -1 = variable absent / fixed. */
typedef struct beatamd_ffi_layout {
    int64_t nparams;
    int32_t nvar;            /* slip variables (uparr, uperp, ...)                        */
    int64_t slip_off[4];     /* [nvar] offset of each slip variable (size npatches)        */
    int64_t durations_off;   /* size npatches                                              */
    int64_t velocities_off;  /* size npatches                                              */
    int64_t nuc_strike_off;  /* size nsubfaults                                            */
    int64_t nuc_dip_off;     /* size nsubfaults                                            */
    int64_t time_off;        /* size nsubfaults                                            */
    int64_t h_laplacian_off; /* size 1, -1 if no laplacian                                 */
} beatamd_ffi_layout;

int beatamd_ffi_model_create(beatamd_ctx *ctx, const beatamd_ffi_layout *layout,
                             int32_t nsubfaults, const int32_t *n_patch_dip,
                             const int32_t *n_patch_strike, const double *patch_size,
                             int32_t *model_id);
/* one seismic wavemap (seismic.py:1274-1341):
 *   lib_ids [nvar]   data [T,N]   wset_id over the T datasets
 *   hp_off [T]: offset in q of each dataset's hyperparameter
 *   shift_off [T]: offset in q of each target's station time-shift, or NULL
 *                  (hierarchicals[time_shifts_id][station_correction_idxs])           */
int beatamd_ffi_model_add_wavemap(beatamd_ctx *ctx, int32_t model_id, const int32_t *lib_ids,
                                  const double *data, int32_t wset_id, const int64_t *hp_off,
                                  const int64_t *shift_off, int32_t interpolation);
/* replaces: the spectrum domain of a wavemap (WaveformFitConfig.domain = "spectrum", beat/heart.py:526) as the
 *           reference's GEOMETRY mode evaluates it: pytensorf.SeisSynthesizer (beat/pytensorf.py:199-206, 294-311),
 *           heart.fft_transforms (beat/heart.py:4091-4155), WaveformMapping.prepare_data (beat/heart.py:3086-3095),
 *           get_valid_spectrum_data (beat/utility.py:1604-1610), get_synthetics (beat/models/seismic.py:932-941).
 *           BEYOND the reference's FFI mode, which stops with TypeError("FFI is currently only supported for
 *           time-domain!") (beat/models/seismic.py:1277-1278): the functions above are what the numbers are pinned to.
 *   A wavemap whose likelihood is formed on amplitude spectra.  The time-domain stack is the one of
 *   beatamd_ffi_model_add_wavemap (seismic.py:1324-1332: sweep, station shifts, interpolation, out-of-grid chains
 *   flagged); per chain c and target t
 *       r[c,t,:] = data_spec[t,:] - abs(rfft(syn[c,t,:], ntrans))[lo:hi]           (zero padded to ntrans)
 *       logpt[c,t] = multivariate_normal_chol with W_t, M = hi - lo samples        beat/models/distributions.py:108-140
 *   data_spec [T,M] is the observed side, transformed by the caller (prepare_data does it with numpy on the host);
 *   wset_id holds T datasets of M samples (scalar, or dense M x M; banded operators are found as for any set).
 *   ntrans = pyrocko.trace.nextpow2(N) = 2^ceil(log2 N) (restated from memory, pyrocko is not in the tree), a power of
 *   two with N <= ntrans, 2 <= ntrans <= 8192; 0 <= lo < hi <= ntrans/2 + 1 -- a band numpy's slice would silently
 *   shorten is BEATAMD_EINVAL here.  Sizes are checked when the wavemap is added.  The covariance of such a dataset is
 *   M x M; the reference's spectral covariances are built at ntrans//2 + 1 bins (beat/covariance.py:133-135) and cut
 *   to [lo:hi] by the caller.
 *   beatamd_ffi_synthetics_batch of such a wavemap returns [C,T,M]: the spectra, or data_spec - spectra.
 *   beatamd_ffi_lsq_* refuse a model with a spectrum wavemap: the problem is not linear in the slips. */
int beatamd_ffi_model_add_wavemap_spectrum(beatamd_ctx *ctx, int32_t model_id, const int32_t *lib_ids,
                                           const double *data_spec, int32_t wset_id, const int64_t *hp_off,
                                           const int64_t *shift_off, int32_t interpolation, int64_t ntrans, int64_t lo,
                                           int64_t hi);
/* replaces: heart.fft_transforms(signals, (lo, hi), outmode="array", pad_to_pow2=True)   beat/heart.py:4091-4155
 *           (one numpy.fft.rfft per trace in a Python loop)
 *   X [R,N] -> out [R, hi - lo] = abs(rfft(X[r], ntrans))[lo:hi], FP64, one real-input FFT per row in LDS
 *   (csrc/spectrum.hip states the operation order); with data_spec [T, hi - lo] (else NULL) out[r] =
 *   data_spec[r mod T] - that.  A row's bits depend on its samples, N, ntrans, lo, hi alone: not on R, the row's
 *   position or data_spec (beyond the subtraction).  Zeros give exact zeros; the padding is never read.
 *   ntrans a power of two, 2 <= ntrans <= 8192, 1 <= N <= ntrans, 0 <= lo < hi <= ntrans/2 + 1, else BEATAMD_EINVAL
 *   and nothing is launched.  Against numpy: |out - numpy| <= 8 max(1, log2 ntrans) 2^-53 |x_r|_2 per bin (tested). */
int beatamd_amp_spectrum_batch(beatamd_ctx *ctx, int64_t R, int64_t N, int64_t ntrans, int64_t lo, int64_t hi,
                               const double *X, const double *data_spec, int64_t T, double *out);
/* geodetic composite (geodetic.py:1065-1081): geo lib per slip var, data [Nobs],
 * odws [Nobs], dataset sizes [nd] (srmap), one wset per dataset (sizes differ) */
int beatamd_ffi_model_add_geodetic(beatamd_ctx *ctx, int32_t model_id, const int32_t *geo_lib_ids,
                                   const double *data, const double *odws, int32_t ndatasets,
                                   const int64_t *dataset_sizes, const int32_t *wset_ids,
                                   const int64_t *hp_off);
/* geometry-mode geodetic composite (GeodeticGeometryComposite.get_formula,
 * beat/models/geodetic.py:605-659): the displacements come from analytic half-space sources
 * instead of a linear GF library -- rectangular dislocations (Okada 1985; kind 0) and Mogi
 * point sources (kind 1) -- then LOS projection (:642), residual * odw and
 * multivariate_normal_chol exactly as above.  The reference obtains the displacements from
 * pyrocko's GF-store engine (heart.geo_synthetics, heart.py:4158-4239; not in its tree):
 * parity with BEAT is unpinned for this entry, it is pinned to Okada's published check values.
 *   per source 10 parameters: east_shift north_shift depth [km] (centre of the top edge),
 *   strike dip rake [deg], length width [km], slip [m] (Mogi: volume change [m^3]),
 *   opening_fraction;  param_off[nsrc*10] = offset in q or -1 -> param_fixed value
 *   east/north [Nobs] observation points [km], los [Nobs,3] = (Sn, Se, Su) (heart.py:1381-1410) */
int beatamd_ffi_model_add_geodetic_geometry(beatamd_ctx *ctx, int32_t model_id, int32_t nsrc,
                                            const int32_t *kind, const int64_t *param_off,
                                            const double *param_fixed, int64_t nobs,
                                            const double *east, const double *north,
                                            const double *los, double nu, const double *data,
                                            const double *odws, int32_t ndatasets,
                                            const int64_t *dataset_sizes, const int32_t *wset_ids,
                                            const int64_t *hp_off);
/* correction terms of the geodetic composite's datasets, the reference's hierarchical dataset corrections
 * (GeodeticComposite.apply_corrections, beat/models/geodetic.py:411-427, called at :1076-1077 between the weighted
 * residual and multivariate_normal_chol; beat/models/corrections.py:46-87 orbital ramp, :143-205 strain rate).
 * Valid once, after add_geodetic / add_geodetic_geometry.  Term j belongs to dataset dataset[j] (its n observations
 * are that dataset's block of the concatenated vector) and has K = ncol[j] basis columns and K coefficients;
 * coefficient k is q[coef_off[j*4+k]], or coef_fixed[j*4+k] where the offset is -1 (lower == upper in the
 * reference, geodetic.py:401-405).  For chain c and observation i of the dataset
 *     corr[c,i] = ((B[i,0]*coef0 + B[i,1]*coef1) + B[i,2]*coef2) + B[i,3]*coef3      plain products and sums
 *     res[c,i]  = ((data[i] - mu[c,i]) * odw[i]) - corr[c,i]                        the term is not weighted
 * and the terms of a dataset are subtracted one after the other in list order (the reference's iter_corrections:
 * ramp, then strain rate).  Ramp: K = 3, B = [locy, locx, 1], coefficients (azimuth_ramp, range_ramp, offset) --
 * bit for bit numpy's expression.  Strain rate: K = 4, the velocity-gradient tensor folded into four columns on
 * the host, coefficients (exx, eyy, exy, rotation) -- equal to the reference to rounding.  The Euler-pole term
 * needs the entry below (this one declares every term linear in entries of q).
 * The subtraction happens in the kernel that forms the residual; the stand-alone synthetics are unchanged.
 *   dataset [nterm] non-decreasing   ncol [nterm] 1..4   coef_off, coef_fixed [nterm*4]
 *   basis: the terms concatenated, term j is dataset_sizes[dataset[j]] x ncol[j], column-major
 * At most 32 terms.  nterm = 0 declares a composite without corrections. */
int beatamd_ffi_model_add_geodetic_corrections(beatamd_ctx *ctx, int32_t model_id, int32_t nterm,
                                               const int32_t *dataset, const int32_t *ncol,
                                               const double *basis, const int64_t *coef_off,
                                               const double *coef_fixed);
/* The same with a kind per term: kind[j] = 0 is the linear term above (the entry above is this one with every kind 0,
 * kind == earth == NULL), kind[j] = 1 the Euler-pole correction (beat/models/corrections.py:90-140,
 * heart.velocities_from_pole beat/heart.py:4326-4392 with earth_shape="ellipsoid", EulerPoleConfig
 * beat/config.py:840-853; in iter_corrections' order, config.py:904-909, between ramp and strain rate).
 * A pole term has K = 3 and its coef_off / coef_fixed slots name (pole_lat, pole_lon, omega) [deg, deg, deg / Myr],
 * each sampled or fixed.  With x_i = ecef(lat_i, lon_i, 0) / r, T_i the ECEF -> NEU rotation (heart.py:4352-4369)
 * and l_i the line of sight (NEU)
 *     corr[c,i] = l_i . T_i (w' p x x_i) = (B[i,0]*coef0 + B[i,1]*coef1) + B[i,2]*coef2
 *     B[i,:] = x_i x (T_i^T l_i)  (host: EulerPoleCorrection.basis(), masked rows zero)      coef = w' p
 *     p = ecef(pole_lat, pole_lon, 0) / r         w' = omega * 1e-6 * (pi / 180) * r
 * so the basis is the caller's as for every term; the three coefficients are derived per chain on the device
 * (k_pole_coef, corrections.hip, which states the order of operations) in front of every kernel that subtracts the
 * table, into a buffer the model owns ([C, npole, 4] doubles, grown with the chain count outside graph captures).
 * earth [nterm*3] = (r, equatorial radius a, oblateness f) of the term's ellipsoid [m, m, 1] (ignored for kind 0):
 * ecef is the closed form N = a / sqrt(1 - e2 sin^2 lat), e2 = 2f - f^2, (N cos lat cos lon, N cos lat sin lon,
 * N (1 - e2) sin lat); a = r, f = 0 is the reference's earth_shape="sphere".  Equal to the reference's evaluation
 * within 16 * 2^-53 * |w'| * |l_i|_1. */
int beatamd_ffi_model_add_geodetic_corrections_kinds(beatamd_ctx *ctx, int32_t model_id, int32_t nterm,
                                                     const int32_t *dataset, const int32_t *ncol,
                                                     const double *basis, const int64_t *coef_off,
                                                     const double *coef_fixed, const int32_t *kind,
                                                     const double *earth);
/* the derived coefficients alone: out [C, npole, 4] = (w' p, 0) of every (row of Q, pole), the kernel the model
 * launches (k_pole_coef).  var_off / var_fixed / earth [npole*3] as above (offset -1: the fixed value) */
int beatamd_pole_coefficients_batch(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q, int32_t npole,
                                    const int64_t *var_off, const double *var_fixed, const double *earth,
                                    double *out);
/* replaces: euler_pole2slips and backslip2coupling, beat/ffi/fault.py:1436-1517, for a batch of draws Q [C, nparams]
 *   of ONE pole (the reference takes the first of several too): var_off / var_fixed / earth [3] as above;
 *   Bp [P, 3] = x_p x (T_p^T s_p) of the patch centres with the strike vectors (NEU) in place of the line of sight
 *   (host: summary.pole_patch_basis; the patch coordinates are the caller's, ne_to_latlon is pyrocko's);
 *   uparr_off: the offset of the P back-slips in q.
 *     euler_slips [C, P] = |(Bp[p,0]*coef0 + Bp[p,1]*coef1) + Bp[p,2]*coef2|            fault.py:1497
 *     coupling    [C, P] = 100 * clip(uparr / euler_slips, 0, 1)                         fault.py:1514-1517
 *   with numpy's IEEE semantics: a NaN ratio stays NaN, x / 0 -> +-inf -> 100 / 0.  Rows are independent: a batch
 *   cut into calls gives the same bits. */
int beatamd_pole_coupling_batch(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q, const int64_t *var_off,
                                const double *var_fixed, const double *earth, int64_t P, const double *Bp,
                                int64_t uparr_off, double *euler_slips, double *coupling);

/* ---- polarity composite (csrc/polarity.hip, which states the order of operations) ----------------------------------
 * Source kinds and their variables, in the order of param_off / param_fixed [6] (offset in q, or -1: the fixed value):
 *   BEATAMD_POL_MTQT  w, v, kappa, sigma, h        MTQTSource at rho = 1, beat/sources.py:19-40, 372-400, 454-536
 *   BEATAMD_POL_MT    mnn, mee, mdd, mne, mnd, med as they are (pyrocko's six-vector order, pinned in the tree by
 *                                                  calculate_radiation_weights == radiation_matmul, heart.py:3891-4050)
 *   BEATAMD_POL_DC    strike, dip, rake [deg]      Aki & Richards; == MTQT(w = v = 0, kappa = strike, sigma = rake,
 *                                                  h = cos dip) after the normalisation
 * utab / btab [ntab]: U_MAPPING and BETA_MAPPING of sources.py:30-36, the caller's data (mtqt only; utab strictly
 * increasing); the device restates numpy.interp on them bit for bit (sources.py:379-392).
 * Every kind is normalised as pol_synthetics does: m9 /= sqrt(sum m9^2) / sqrt 2 (heart.py:4086-4087). */
#define BEATAMD_POL_MTQT 0
#define BEATAMD_POL_MT 1
#define BEATAMD_POL_DC 2
/* replaces: PolarityComposite.get_formula, beat/models/polarity.py:104-134 (PolaritySynthesizer, pytensorf.py:314-369,
 *           with is_location_fixed; pol_synthetics, heart.py:4053-4088; polarity_llk, models/distributions.py:143-173)
 *   nmap polarity maps (at most 8) of n_t[i] stations; rw [6, NT] their propagation coefficients side by side
 *   (NT = sum n_t; heart.py:3891-3958), obs [NT] the observed polarities (+1, -1 or 0) as doubles; gamma the
 *   probability of a wrong reading (polarity.py:45); hp_off / hp_fixed [nmap]: the map's sigma in q, or -1 and its
 *   fixed value -- used as it is, not through exp.
 *   The composite adds NT columns to LL (polarity_like is a vector, polarity.py:133), behind the geodetic ones and in
 *   front of the laplacian's, as one group of the `like` sum.  One launch per evaluation.  It has no Gaussian misfit:
 *   beatamd_ffi_llks_batch, ..._obs_quads, ..._variance_reductions_batch and the lsq entries refuse such a model. */
int beatamd_ffi_model_add_polarity(beatamd_ctx *ctx, int32_t model_id, int32_t kind, const int64_t *param_off,
                                   const double *param_fixed, int32_t nmap, const int64_t *n_t, const double *rw,
                                   const double *obs, double gamma, const int64_t *hp_off, const double *hp_fixed,
                                   int64_t ntab, const double *utab, const double *btab);
/* replaces: MTQTSource.m6 (sources.py:538-540) / a source's pyrocko_moment_tensor().m6() followed by the normalisation
 *           of heart.py:4086-4087, for a population: Q [C, nparams] -> m6 [C, 6] */
int beatamd_mt6_batch(beatamd_ctx *ctx, int32_t kind, int64_t C, int64_t nparams, const double *Q, const int64_t *param_off,
                      const double *param_fixed, int64_t ntab, const double *utab, const double *btab, double *m6);
/* replaces: heart.pol_synthetics, heart.py:4053-4088, for a population: amplitudes [C, NT] = rw.T . m6 */
int beatamd_polarity_amplitudes_batch(beatamd_ctx *ctx, int32_t kind, int64_t C, int64_t nparams, const double *Q,
                                      const int64_t *param_off, const double *param_fixed, int64_t ntab, const double *utab,
                                      const double *btab, int64_t NT, const double *rw, double *amplitudes);
/* replaces: sources.w_to_beta, sources.py:379-392: beta [n] = numpy.interp(3 pi / 8 - w, utab, btab), bit for bit */
int beatamd_w_to_beta_batch(beatamd_ctx *ctx, int64_t n, const double *w, int64_t ntab, const double *utab, const double *btab,
                            double *beta);
int beatamd_ffi_model_set_laplacian(beatamd_ctx *ctx, int32_t model_id, int32_t lap_id);
int beatamd_ffi_model_nllk(beatamd_ctx *ctx, int32_t model_id, int64_t *nllk);
int beatamd_ffi_model_destroy(beatamd_ctx *ctx, int32_t model_id);

/* replaces: SeismicComposite.get_synthetics(point) for the distributed-slip composite
 *           (sweep -> start times -> stack_all), beat/models/seismic.py:1351-1507, as
 *           update_weights / analyse_noise call it at the MAP point of a stage (:1509-1534,
 *           beat/covariance.py:333-395)
 *   Q [C,nparams] -> out [C,T,N] of wavemap `wavemap_index`: synthetics, or (residuals != 0)
 *   data - synthetics (seismic.py:1332).  An index outside the library is BEATAMD_EINDEX; the rows of
 *   such a chain are then UNSPECIFIED (they differ between the stacking kernels; the reference raises
 *   IndexError before producing any). */
int beatamd_ffi_synthetics_batch(beatamd_ctx *ctx, int32_t model_id, int32_t wavemap_index, int64_t C,
                                 const double *Q, int32_t residuals, double *out);

/* logp_forw_func batched: Q [C,nparams] -> LL [C,nllk] */
int beatamd_ffi_logp_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q,
                           double *LL);

/* replaces: Metropolis.astep for C chains at once   beat/sampler/metropolis.py:276-422
 *           (stage > 0, check_bound=True, continuous variables)
 *   Q0 [C,nparams] current points (updated in place)
 *   L0 [C,nllk]    current likelihood vectors = chain_previous_lpoint (updated in place)
 *   delta [C,nparams] proposal_samples_array[stage_sample] rows
 *   scaling [C]    per-chain step scaling;  lower/upper [nparams] Uniform prior boxes
 *   log_u [C]      log of the MH uniforms (metrop_select)
 *   beta           tempering parameter;  accepted [C] int32 out (1 = moved)            */
int beatamd_ffi_astep_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0,
                            double *L0, const double *delta, const double *scaling,
                            const double *lower, const double *upper, const double *log_u,
                            double beta, int32_t *accepted);
/* same with one beta per chain: the replicas of a parallel-tempering ladder
 * (worker_process / sample_pt_chain, beat/sampler/pt.py:651-790) advance in one batch */
int beatamd_ffi_astep_batch_betas(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0,
                                  double *L0, const double *delta, const double *scaling,
                                  const double *lower, const double *upper, const double *log_u,
                                  const double *betas, int32_t *accepted);

/* The whole Metropolis step with the proposal drawn on the device: what the two calls
 * beatamd_proposal_draw[_univariate] + beatamd_ffi_astep_batch[_betas] do, as one call that touches
 * the host for nothing (the sampling loop of a stage is then one C call per step, capturable in a
 * HIP graph together with the device-resident step counter, beatamd_ctx_set_step_counter).
 * replaces: Metropolis.astep incl. its proposal draw and bookkeeping
 *           beat/sampler/metropolis.py:276-422 (proposal_dist(n_steps) :289-292, accepted :386-410)
 *   factor, K, kind, df   kind -1: multivariate proposal, factor [K,nparams], delta = z.factor
 *                         (df > 0: multivariate-t row scale, base.py:35-71);
 *                         kind 0/1/2: per-parameter Normal/Cauchy/Laplace, factor = scales [nparams]
 *   seed, step, first_chain   the Philox key/counter of beatamd_proposal_draw (same numbers)
 *   beta / betas          betas != NULL: one beta per chain (parallel tempering), else the scalar
 *   accepted [C] int32 out; accepted_sum [C] int32 (+= accepted) and n_accepted [1] int64
 *   (+= number of moves) may be NULL.  Q0, L0 and the counters are device pointers.
 * For nparams, K <= 64 the draws, the factor product and the prior-box test are one launch.       */
int beatamd_ffi_mstep_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0, double *L0,
                            const double *factor, int64_t K, int32_t kind, int32_t df, uint64_t seed,
                            uint32_t step, int64_t first_chain, const double *scaling,
                            const double *lower, const double *upper, double beta, const double *betas,
                            int32_t *accepted, int32_t *accepted_sum, int64_t *n_accepted);

/* ---------------------------------------------------------------- noise covariance -------
 * Per-stage re-estimation of the data covariances (update_weights with the "non-toeplitz"
 * structure, seismic.py:1509-1534 -> covariance.py:397-427): the reference runs O(n^2) Python
 * loops per dataset.
 * replaces: covariance.autocovariance(data)            beat/covariance.py:716-736
 *   data [nd,n], mean [nd] (= data.mean(), computed by the caller) or NULL (each row's mean
 *   is then taken on the device in numpy's summation order: numpy.mean to the bit) -> out [nd,n]
 *   same term order as the reference loop: bitwise equal results                             */
int beatamd_autocovariance_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *data,
                                 const double *mean, double *out);
/* replaces: toeplitz(coeffs) * stds[:,None] * stds[None,:]   beat/covariance.py:739-771
 *   coeffs [nd,n], stds [nd,n] -> out [nd,n,n]                                               */
int beatamd_scaled_toeplitz_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *coeffs,
                                  const double *stds, double *out);

/* replaces: covariance.k_nearest_neighbor_rms(coords, data, max_dist_perc=...)   beat/covariance.py:774-811
 *           (the max_dist_perc branch; what GeodeticNoiseAnalyser.do_non_toeplitz :193-210 reaches through
 *           non_toeplitz_covariance_2d :831-848 and toeplitz_covariance_2d :814-828 for every SAR scene when
 *           GeodeticDistributerComposite.update_weights, geodetic.py:1145-1148, re-estimates the data covariances)
 *   nd datasets of sizes[i] points, concatenated: coords [Ntot, 2] (east, north), data [Ntot] -> radius [nd],
 *   counts [Ntot] (neighbours of each point, itself included), stds [Ntot].  Arrays may live on either side.
 *   THE ORDER, per dataset of n points, plain products and sums (no contraction):
 *       d2(i,j) = dx*dx + dy*dy;   radius = sqrt(max_ij d2) * max_dist_perc  (sqrt correctly rounded: bit for bit
 *       utility.distances(coords, coords).max() * max_dist_perc);   j neighbours i iff d2(i,j) <= radius*radius
 *       (the same sets as scipy's KDTree.query_ball_point, exact ties included);
 *       a sum over the neighbours of i: 64 partials, partial l takes the neighbours j == l (mod 64) in ascending j
 *       from 0, then partial[l] += partial[l + h] for l < h, h = 32, 16, 8, 4, 2, 1;
 *       mean = sum(x_j) / count;   stds[i] = sqrt(sum((x_j - mean)^2) / (count - 1));   count < 2: NaN (as numpy.std
 *       with ddof = 1).
 *   It depends on (i, n) alone -- not on the launch geometry, not on the other datasets of the call.  The KD-tree
 *   returns neighbours in no defined order, so the reference's last bits are not defined either: stds agree with it
 *   to (count + 3) 2^-53 relative.  nd <= 0, a dataset of size 0 and a non-finite max_dist_perc: BEATAMD_EINVAL. */
int beatamd_ball_rms_batch(beatamd_ctx *ctx, int64_t nd, const int64_t *sizes,
                           const double *coords /* [Ntot, 2] east, north */,
                           const double *data /* [Ntot] */, double max_dist_perc,
                           double *radius /* [nd] */, int32_t *counts /* [Ntot] */,
                           double *stds /* [Ntot] */);

/* ---------------------------------------------------------------- SMC stage transition ----
 * The population (end points Q [C,nparams], likelihood vectors L [C,nllk]) stays in HBM between
 * stages; these entries run on device pointers (host pointers are staged like everywhere else).
 * All reductions have a fixed order, so every rank of a multi-GPU run that holds the same gathered
 * arrays computes bit-identical decisions.
 *
 * replaces: SMC.calc_beta                                   beat/sampler/smc.py:133-165
 *   likelihoods: C values `stride` doubles apart (the `like` column of L: stride = nllk)
 *   -> *beta_new (host), weights [C] (importance weights of the last bisection midpoint,
 *      normalised).  exp() is the device's (<= 1 ulp from glibc/numpy): weights agree with
 *      the reference to ~1e-15 relative, beta exactly unless a bisection decision sits on a tie.
 *   beta must leave an interval to halve, 2 - beta > 1e-6 (the reference's loop condition; it has
 *   nothing to return otherwise): BEATAMD_EINVAL. */
int beatamd_smc_calc_beta(beatamd_ctx *ctx, int64_t C, const double *likelihoods, int64_t stride,
                          double beta, double coef_variation, double *beta_new, double *weights);
/* final stage (smc.py:526-529): weights = exp(dbeta (l - max l)) / sum */
int beatamd_smc_stage_weights(beatamd_ctx *ctx, int64_t C, const double *likelihoods, int64_t stride,
                              double dbeta, double *weights);
/* replaces: SMC.resample (Kitagawa's deterministic resampling)   beat/sampler/smc.py:290-324
 *   weights [C], aux = the single uniform draw (host RNG, shared by all ranks)
 *   -> indexes [C] int32 = np.repeat(parents, N_childs); sequential cumulative sum as np.cumsum:
 *      bit-exact indices */
int beatamd_smc_resample(beatamd_ctx *ctx, int64_t C, const double *weights, double aux,
                         int32_t *indexes);
/* replaces: SMC.calc_covariance + MultivariateNormalProposal   smc.py:167-186, base.py:163-167
 *   factor [C,nparams] with factor^T factor = np.cov(population, aweights=weights, bias=False):
 *   rows z . factor (z ~ N(0, I_C)) are draws of N(0, cov) without factoring the covariance */
int beatamd_smc_population_factor(beatamd_ctx *ctx, int64_t C, int64_t nparams,
                                  const double *population, const double *weights, double *factor);
/* replaces: proposal_dist(n_steps) rows + the Metropolis uniforms   metropolis.py:289-292, 355-358
 *           multivariate_t_rvs                                       base.py:35-71
 *   delta [C,nparams] = z [C,K] . factor [K,nparams] (FP64 MFMA), z from Philox4x32-10 keyed by
 *   `seed` with counter (pair, first_chain + c, step, stream): a chain's draws do not depend on
 *   the sharding.  df = 0: multivariate normal; df > 0: multivariate t (1 = Cauchy): rows divided
 *   by sqrt(chi2(df) / df).  log_u [C] (nullable) = log of U(0,1). */
int beatamd_proposal_draw(beatamd_ctx *ctx, int64_t C, int64_t K, int64_t nparams,
                          const double *factor, uint64_t seed, uint32_t step, int64_t first_chain,
                          int32_t df, double *delta, double *log_u);
/* replaces: NormalProposal / CauchyProposal / LaplaceProposal / PoissonProposal (per-parameter families)
 *                                                              beat/sampler/base.py:129-160
 *   delta [C,nparams]: every component an independent draw times scale[j] (the reference's
 *   Metropolis passes scale = ones, metropolis.py:209-212); same Philox counters as above
 *   (streams 3, 4); log_u [C] (nullable) = log of U(0,1).  Poisson: poisson(lam = scale[j]) - scale[j]
 *   (inversion of one uniform by sequential search; scale[j] <= 500, NaN rows beyond). */
#define BEATAMD_PROPOSAL_NORMAL 0
#define BEATAMD_PROPOSAL_CAUCHY 1
#define BEATAMD_PROPOSAL_LAPLACE 2
#define BEATAMD_PROPOSAL_POISSON 3   /* poisson(lam = scale) - scale (beat/sampler/base.py:150-155) */
int beatamd_proposal_draw_univariate(beatamd_ctx *ctx, int64_t C, int64_t nparams, int32_t kind,
                                     const double *scale, uint64_t seed, uint32_t step, int64_t first_chain,
                                     double *delta, double *log_u);
/* out[i,:] = src[indexes[i],:]: chains restart at their resampled parents (sampler/base.py:541-571),
 * replica exchange permutation (pt.py:573-633).  An index outside [0,nrows_src) is BEATAMD_EINDEX
 * at the next synchronisation. */
int beatamd_gather_rows(beatamd_ctx *ctx, int64_t nout, int64_t ncols, const double *src,
                        int64_t nrows_src, const int32_t *indexes, double *out);
/* ---- a Metropolis step in pieces, for models with a collective between forward model and acceptance (libraries sharded
 * by TARGET over ranks; beat_amd/models/sharded.py).  All pointers are device pointers.
 *
 * beatamd_like_assemble: the full likelihood vectors LL [C, nllk] (layout of the unsharded model: datasets..., like) from
 *   the all-gathered block `gathered` [nsrc, C] -- row r goes to column dst_col[r] (host int32 [nsrc]); dst_col[r] = -1
 *   marks a rank's FLAG row (NaN in it = that rank saw the chain's start times / durations leave the library grid: the
 *   reference raises IndexError there, beat/ffi/base.py:486-568) -- + the replicated columns (geodetic datasets,
 *   Laplacian) local_ll[c*local_ld + local_col0 .. +n_rest) -> columns rest_dst0..; then like = the composites' sums in
 *   order, summed (beat/models/problems.py:227-247; group_end [ngroups] host: exclusive column ends), NaN for flagged chains.
 * beatamd_metropolis_propose: q = q0 + delta * scaling, prior box test, out-of-box rows parked on q0 (metropolis.py:313-343).
 * beatamd_metropolis_accept: tempered acceptance iff in bounds, isfinite(mr), log u < mr with mr = beta (like' - like)
 *   (betas [C] non-NULL: per chain) -- metropolis.py:344-385 + pymc metrop_select; Q0 / L0 updated in place. */
int beatamd_like_assemble(beatamd_ctx *ctx, int64_t C, int64_t nllk, int64_t nsrc, const double *gathered,
                          const int32_t *dst_col, const double *local_ll, int64_t local_ld, int64_t local_col0,
                          int64_t n_rest, int64_t rest_dst0, int32_t ngroups, const int32_t *group_end, double *LL);
int beatamd_metropolis_propose(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q0, const double *delta,
                               const double *scaling, const double *lower, const double *upper, double *Qprop,
                               int32_t *inbounds);
int beatamd_metropolis_accept(beatamd_ctx *ctx, int64_t C, int64_t nparams, int64_t nllk, double *Q0, double *L0,
                              const double *Qprop, double *Lprop, const int32_t *inbounds, const double *log_u, double beta,
                              const double *betas, int32_t *accepted);
/* replaces: the per-chain step-size tuning of Metropolis.astep   metropolis.py:294-306
 *   scaling [C] *= pymc's tune factor of accepted[c] / tune_interval; accepted [C] reset to 0 */
int beatamd_metropolis_tune(beatamd_ctx *ctx, int64_t C, double *scaling, int32_t *accepted,
                            int32_t tune_interval);

/* ---------------------------------------------------------------- hyper-parameter estimation ----
 * `beat sample --hypers`: the source is fixed at one point per chain, each dataset's whitened misfit |W r|^2 is
 * cached once, and Metropolis runs on the noise scalings h_* alone (estimate_hypers, beat/models/base.py:304-379;
 * init_chain_hypers, beat/sampler/base.py:398-418; built_hyper_model, beat/models/problems.py:261-297).
 *
 * replaces: update_llks of every composite for C points at once
 *           beat/models/seismic.py:510-525, beat/models/geodetic.py:429-444, beat/models/laplacian.py:141-154
 *   Q [C,nparams] -> llks [C,nterm] (host or device pointers): one column per seismic dataset (wavemap by wavemap),
 *   one per geodetic dataset, ONE PER SLIP VARIABLE of the Laplacian (|L s_v|^2; the likelihood sums these into one
 *   laplacian_like, the hyper model keeps them apart, laplacian.py:151-170); nterm from beatamd_ffi_model_nterm.
 *   The values are the quadratic forms the likelihood hands to its epilogues, from the same kernels (scalar and
 *   bidiagonal covariances in the stacking epilogue, dense W in the matrix-core quadratic form, pre-whitened
 *   libraries, the small-dataset geodetic kernel, the geometry-mode composite); station time shifts and dataset
 *   corrections are part of the residual as in the likelihood.  The hyper-parameter entries of Q are not read.
 *   A chain whose times leave the library grid gets NaN in all its columns and raises the status word as
 *   beatamd_ffi_logp_batch does.
 *   DEVIATION: the reference's geodetic update_llks forms data - synthetics WITHOUT the odw factor
 *   (geodetic.py:221, 439-443) although its likelihood uses (data - mu) * odw (:1072).  Here the cached misfit is
 *   the likelihood's own, so that the hyper model IS the full model at a fixed source point; with odw = 1 the two
 *   agree. */
int beatamd_ffi_model_nterm(beatamd_ctx *ctx, int32_t model_id, int64_t *nterm);
int beatamd_ffi_llks_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *llks);
/* replaces: hyper_normal                      beat/models/distributions.py:176-222 (through
 *           Composite.get_hyper_formula, beat/models/base.py:110-123) and the Laplacian's _eval_prior /
 *           get_hyper_formula, beat/models/laplacian.py:88-96, 156-170
 *   Term k reads hyper-parameter hp_index[k] of the nh-vector (get_hyper_name / Counter order, distributions.py:24-25,
 *   195-210):
 *     kind 0 (dataset)    -0.5 * (slog[k] + (M[k] * 2 * h) + (1 / exp(h * 2)) * llk)         no M log 2pi; M uncast
 *     kind 1 (Laplacian)  -0.5 * (-slog[k] + (M[k] * (LOG_2PI + 2 * h)) + (1 / exp(h * 2) * llk))
 *   in this operation order.  group_end [ngroups <= 8]: exclusive ends of the composites inside the term vector;
 *   like = the composites' sums added in composite order (problems.py:286-296), each composite summed by a fixed
 *   rule of (nterm, group_end) alone: 64 strided partial sums (term k to partial k mod 64, ascending), joined by a
 *   butterfly (xor 32, 16, ..., 1).  M, slog, kind, hp_index, group_end are host arrays.  At most 2048 terms. */
int beatamd_hyper_model_create(beatamd_ctx *ctx, int64_t nterm, int64_t nh, const int64_t *M, const double *slog,
                               const int32_t *kind, const int32_t *hp_index, int32_t ngroups, const int32_t *group_end,
                               int32_t *id);
int beatamd_hyper_model_destroy(beatamd_ctx *ctx, int32_t id);
/*   H [C,nh], llks [C,nterm] -> LL [C,nterm+1]: the terms, then like (host or device pointers) */
int beatamd_hyper_logp_batch(beatamd_ctx *ctx, int32_t id, int64_t C, const double *H, const double *llks, double *LL);
/* replaces: n_steps calls of Metropolis.astep per chain       beat/sampler/metropolis.py:294-306, 313-385
 *   ALL n_steps steps of all C chains in ONE launch (the chains are independent: one wavefront each, no barrier
 *   between them).  Device pointers only.  In / out: H [C,nh], LL [C,nterm+1], scaling [C], accepted_since_tune [C];
 *   in: llks [C,nterm], lower / upper [nh], kind 0/1/2 (Normal / Cauchy / Laplace) with scales [nh]; out: trace
 *   [ndraws, C, nh+nterm+1] (nullable) and n_accepted [1] (+= moves, nullable).
 *   Step s is step step0 + s of the step-by-step path (beatamd_proposal_draw_univariate, beatamd_metropolis_propose,
 *   beatamd_hyper_logp_batch, beatamd_metropolis_accept with beta = 1, beatamd_metropolis_tune) for chain
 *   first_chain + c, bit for bit: the same Philox counters and transforms, q = q0 + delta * scaling, a proposal outside
 *   the box is rejected without evaluation, accept iff isfinite(mr) and log u < mr.  tune_interval > 0: the tune table
 *   is applied in front of a step whenever steps_until_tune has run down to 0 (then reset to tune_interval);
 *   tune_interval = 0: no tuning.  The draw after step s is recorded iff (n_steps - 1 - s) % buffer_thinning == 0 -- the
 *   reference's buffer[-1::-buffer_thinning] reversed (thin_buffer, beat/backend.py:100-118, with the whole run in
 *   the buffer): ndraws = ceil(n_steps / buffer_thinning).
 *   A chain's wavefront holds at most 1024 hyper-parameters and 1024 terms: beyond that BEATAMD_EINVAL (take the
 *   step-by-step path). */
int beatamd_hyper_chain_batch(beatamd_ctx *ctx, int32_t id, int64_t C, int64_t n_steps, double *H, double *LL,
                              double *scaling, int32_t *accepted_since_tune, const double *llks, const double *lower,
                              const double *upper, int32_t kind, const double *scales, uint64_t seed, uint32_t step0,
                              int64_t first_chain, int32_t tune_interval, int32_t steps_until_tune, int32_t buffer_thinning,
                              double *trace, int64_t *n_accepted);

/* ---------------------------------------------------------------- posterior diagnostics ----
 * What a BEAT project asks of a finished stage -- variance reductions, standardized residuals, the synthetics of
 * an ensemble of draws -- for whole populations at once (the reference runs one forward model per draw).
 *
 * replaces: the quadratic forms residual.T.dot(icov).dot(residual) / data.T.dot(icov).dot(data) of
 *           get_variance_reductions           beat/models/seismic.py:610-616, beat/models/geodetic.py:494-501
 *   quad[c,d] = |W_d R[c,d,:]|^2 for a weight set (W^T W = inv(C)), through the misfit kernels of
 *   beatamd_mvn_chol_logp_batch: scalar, banded and dense.   R [C, nd, M] -> quad [C, nd] */
int beatamd_wset_quad_batch(beatamd_ctx *ctx, int32_t wset_id, int64_t C, const double *R, double *quad);
/* replaces: denom = data.T.dot(icov).dot(data) per dataset   seismic.py:612-616, geodetic.py:497-501
 *   denom [ndata] = |W_k d_k|^2 of every dataset of the model, in the order of the first ndata columns of
 *   beatamd_ffi_llks_batch (seismic datasets wavemap by wavemap, then the geodetic ones; no Laplacian columns):
 *   beatamd_wset_quad_batch on the model's own data as a one-chain batch.  A pre-whitened wavemap holds whitened data:
 *   |d'|^2.  Computed once and kept on the model until beatamd_weights_update, beatamd_ffi_model_update_data, a
 *   (re-)whitening of library rows or beatamd_ffi_model_add_geodetic_corrections.
 *   DEVIATION (as for beatamd_ffi_llks_batch): geodetic data carries the odw factor, d_k * odw_k, like the residual
 *   of the likelihood; the reference's variance reduction leaves odw out (geodetic.py:221). */
int beatamd_ffi_obs_quads(beatamd_ctx *ctx, int32_t model_id, double *denom);
/* replaces: get_variance_reductions(point) per draw, as form_result_ensemble and `beat summarize` loop it
 *           beat/models/seismic.py:564-634, beat/models/geodetic.py:446-511,
 *           beat/plotting/seismic.py:395-451, beat/plotting/geodetic.py:194-227, 580-610
 *   Q [C,nparams] -> VR [C,ndata] = 1 - nom / denom: nom = the misfits of beatamd_ffi_llks_batch, denom =
 *   beatamd_ffi_obs_quads, plain IEEE arithmetic (a zero denominator gives what the division gives).  The
 *   hyper-parameter entries of Q are not read: inverse(exp(2h)) scales numerator and denominator alike.  A chain
 *   whose times leave the library grid gets a NaN row and raises the status word as beatamd_ffi_llks_batch does. */
int beatamd_ffi_variance_reductions_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *VR);
/* replaces: the geodetic residual / synthetics of a point     beat/models/geodetic.py:1065-1077 (FFI),
 *           :605-659 (geometry), as get_standardized_residuals / get_variance_reductions need them (:446-543)
 *   Q [C,nparams] -> out [C, nobs_total]: residuals != 0: the likelihood's own residual (d - mu) * odw - corrections
 *   (geodetic.py:1072-1077); residuals == 0: mu.  The stacking and residual kernels of the likelihood. */
int beatamd_ffi_geo_residuals_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, int32_t residuals,
                                    double *out);
/* replaces: choli = inv(covariance.chol(exp(hp * 2))); choli.dot(ydata)
 *           get_standardized_residuals       beat/models/seismic.py:527-562, beat/models/geodetic.py:513-543
 *   out[c,t,:] = exp(-hp[c,t]) * (S_t . R[c,t,:]) with S_t = inv(chol(C_t)) handed in (lower triangular in the
 *   reference; any matrix is accepted -- this is NOT the whitening operator chol(inv(C)).T of a weight set):
 *   kind BEATAMD_W_SCALAR: S [T] (1 / sigma_t), BEATAMD_W_DENSE: S [T,N,N] row-major.  R, out [C,T,N]; hp [C,T] or
 *   NULL (no scale).  The dense product runs on the FP64 matrix cores (the GEMM of beatamd_whiten_rows), every
 *   output element summed over k in a fixed order; out must not alias R for a dense operator. */
int beatamd_standardize_batch(beatamd_ctx *ctx, int32_t kind, const double *S, int64_t T, int64_t N, int64_t C,
                              const double *R, const double *hp, double *out);
/* replaces: collecting processed_syn of every ensemble member and reducing them on the host
 *           form_result_ensemble             beat/plotting/seismic.py:395-451
 *   Running column moments of X [C,M] (a batch of synthetics [C, T*N] as it leaves beatamd_ffi_synthetics_batch):
 *   state [5,M] = (mean, M2, min, max, rows seen); n_seen = rows folded in before this call (0: the state is
 *   initialised, its content is not read).  Rows are taken in row order with exactly
 *       d = x - m;  m = m + d / n;  M2 = M2 + d * (x - m)
 *   so the result is bit for bit independent of how the rows are cut into calls.  A NaN makes its column's mean and
 *   std NaN; min and max of such a column are unspecified.
 *   finish: mean, std = sqrt(M2 / n) (numpy.std with ddof = 0), min, max [M] after n rows. */
int beatamd_ensemble_moments_update(beatamd_ctx *ctx, int64_t C, int64_t M, const double *X, double *state,
                                    int64_t n_seen);
int beatamd_ensemble_moments_finish(beatamd_ctx *ctx, int64_t M, const double *state, int64_t n, double *mean,
                                    double *std, double *min, double *max);
/* replaces: fuzzy_waveforms' loop of draw_line_on_array over the traces of an ensemble
 *           beat/plotting/seismic.py:255-316 (used at :503 with linewidth=7, grid_size=(500, 500)),
 *           draw_line_on_array / _weighted_line   beat/plotting/common.py:619-801,
 *           positions2idxs                        beat/utility.py:1556
 *   Y [E,T,N] (synthetics as they leave beatamd_ffi_synthetics_batch), sample j of target t at time tmin[t] + j * deltat,
 *   extent [T,4] = (xmin, xmax, ymin, ymax) per target, grid [T,ny,nx] (rows = amplitude, columns = time): every trace is
 *   drawn as N - 1 anti-aliased segments of width `linewidth` into an image of its own, a pixel keeping the value of
 *   the last segment that writes it, and the image is ADDED to grid[t]; traces in ensemble order.  Cell indices are
 *   round((pos - min - step / 2) / step), half to even, step = (max - min) / (n - 1); the last row and the last column
 *   are never written (the reference's limits).  All arithmetic is the reference's, operation by operation: the grid
 *   equals draw_line_on_array's bit for bit, however the ensemble is cut into calls.
 *   BEATAMD_EOUTSIDE (TypeError, check_line_in_grid): an index above ny - 1 / nx - 1.  Negative indices are clipped.
 *   DEVIATIONS: a sample or extent that is not finite (or xmax <= xmin) is BEATAMD_EINVAL -- the reference casts NaN to an
 *   arbitrary int32; an index below -32768 is BEATAMD_EOUTSIDE -- the reference's int32 products overflow there.
 *   BEATAMD_EINVAL also for ny, nx outside 2 ... 4096, linewidth outside (0, 64], N < 2, deltat <= 0.  The call
 *   synchronises to report these; after an error the grid is unspecified. */
int beatamd_trace_density_update(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin,
                                 double deltat, const double *extent, int64_t ny, int64_t nx, double linewidth,
                                 double *grid);
/* replaces: fuzzy_moment_rate's loop of draw_line_on_array over moment-rate functions that each cover their own stretch
 *           of the time axis                      beat/plotting/ffi.py:41-79
 *   beatamd_trace_density_update with ranges [E,T,2] (int64) = (first sample, count) of every trace: only the segments
 *   between samples inside a trace's own range are drawn (zero padding would add segments along rate 0), only those
 *   samples are checked against the extent, and a trace with count < 2 draws nothing.  A range is cut to [0, N).
 *   ranges == NULL: beatamd_trace_density_update itself, bit for bit. */
int beatamd_trace_density_update_ranges(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin,
                                        double deltat, const double *extent, const int64_t *ranges, int64_t ny, int64_t nx,
                                        double linewidth, double *grid);

/* ---------------------------------------------------------------- library whitening ------
 * rows [nrows, N] (device, in place) <- rows . W^T, W [N,N] = chol_inverse of one dataset: the
 * dense W.r of multivariate_normal_chol (distributions.py:128) applied once to every library row
 * of the dataset instead of once per chain step (SeismicWavemap.prewhitened).  FP64 MFMA GEMM;
 * an upper-triangular W (heart.py:233) skips its zero half. */
int beatamd_whiten_rows(beatamd_ctx *ctx, double *rows, int64_t nrows, int64_t N, const double *W);
/* the same for all datasets of a wavemap in one call: rows [nbatch, nrows, N] (device, in place),
 * W [nbatch, N, N] (host or device).  Upper-triangular operators are applied column block by column block
 * in ascending order with no second buffer (a product column n needs the row's entries k >= n only);
 * anything else goes dataset by dataset through beatamd_whiten_rows.  This is what a covariance update of
 * a pre-whitened model costs per stage (seismic.py:1509-1534 on 62.9 GB of rows at config 3). */
int beatamd_whiten_rows_batch(beatamd_ctx *ctx, double *rows, int64_t nbatch, int64_t nrows, int64_t N,
                              const double *W);

/* ---------------------------------------------------------------- whitening operator ------
 * replaces: heart.Covariance.chol_inverse / .log_pdet                beat/heart.py:216-253
 *           (numpy.linalg.inv + cholesky, + slogdet) for a stack of nd covariance matrices, as
 *           update_weights needs them per stage for every dataset (seismic.py:1509-1534)
 *   covs [nd,n,n] symmetric positive definite -> W [nd,n,n] = cholesky(inv(C)).T (upper
 *   triangular), log_pdet [nd] = log det C.  Blocked factorisation of the exchange-flipped matrix
 *   on the FP64 matrix cores (no explicit inverse of C).  A matrix that is not positive definite
 *   is BEATAMD_ENOTPSD (numpy raises LinAlgError). */
int beatamd_chol_inverse_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *covs, double *W,
                               double *log_pdet);
/* same, for callers that repair the failing matrices themselves (utility.ensure_cov_psd /
 * repair_covariance, beat/utility.py:1034-1138; get_data_covariances, beat/covariance.py:413-427):
 * not_psd [nd] = 1 where the factorisation met a non-positive pivot (W / log_pdet of that matrix
 * are meaningless), no error is raised. */
int beatamd_chol_inverse_batch_flags(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *covs, double *W,
                                     double *log_pdet, int32_t *not_psd);

/* replaces: the Cholesky factor inside pymc's MultivariateNormalProposal (base.py:163-186,
 *           numpy.linalg.cholesky of the proposal covariance) for the stage proposals of SMC:
 *   factor [K,n] (beatamd_smc_population_factor, K = number of chains) -> R [n,n] upper triangular
 *   with R^T R = factor^T factor, so that z[n] . R has the distribution of z[K] . factor.  Used when
 *   the population is larger than the number of parameters (n normals per proposal row instead
 *   of K).  A Gram matrix that is not numerically positive definite is BEATAMD_ENOTPSD: the caller
 *   keeps the tall factor (a collapsed or too small population). */
int beatamd_factor_compact(beatamd_ctx *ctx, int64_t K, int64_t n, const double *factor, double *R);

/* replaces: nothing in the reference (it keeps W and multiplies per step); companion of
 *           beatamd_whiten_rows for update_weights (seismic.py:1509-1534) on a pre-whitened library:
 *   M [nd,n,n] = W_new . inv(W_old) for upper-triangular whitening operators, so that
 *   rows . W_new^T = (rows . W_old^T) . M^T -- the library and the data follow a covariance update in
 *   place.  A singular W_old is BEATAMD_ENOTPSD. */
int beatamd_whitening_ratio_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *W_new,
                                  const double *W_old, double *M);
/* replaces: nothing in the reference; the covariance update (covariance.py:307-325 estimates the noise on
 *           d - s) on a pre-whitened model, whose residual traces are W_old (d - s):
 *   X [nd,n] <- inv(W_t) . X[t] for upper-triangular W [nd,n,n] (back substitution, one trace per
 *   dataset; in place, host or device pointers).  A zero on a diagonal is BEATAMD_ENOTPSD. */
int beatamd_unwhiten_traces(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *W, double *X);
/* replaces: the data half of update_weights on a pre-whitened wavemap: new observed data
 *   [T,N] (already whitened) of wavemap `wavemap_index` of a compiled model */
int beatamd_ffi_model_update_data(beatamd_ctx *ctx, int32_t model_id, int32_t wavemap_index, const double *data);

/* ---------------------------------------------------------------- half-space synthetics ---
 * replaces: heart.geo_synthetics(engine, targets, sources, outmode)   beat/heart.py:4158-4239
 *           (what pytensorf.GeoSynthesizer.perform calls, pytensorf.py:88-123) for a HOMOGENEOUS
 *           HALF SPACE: rectangular dislocations (Okada 1985; kind 0) and Mogi sources (kind 1).
 *           The reference computes these displacements with pyrocko's layered GF-store engine
 *           (not in its tree): parity with BEAT is unpinned for this entry, it is pinned to Okada's
 *           published check values.
 *   params [C, nsrc, 10]: east_shift north_shift depth [km] (top-edge centre), strike dip rake
 *   [deg], length width [km], slip [m] (Mogi: volume change [m^3]), opening_fraction
 *   east/north [nobs] observation points [km]
 *   -> out [C, nsrc, nobs, 3] = (north, east, up) displacement [m] of every source at every point
 *      (the reference's per-(source, target) arrays `[n, e, -d]`, heart.py:4218-4224) */
int beatamd_halfspace_displacements_batch(beatamd_ctx *ctx, int64_t C, int32_t nsrc,
                                          const int32_t *kind, const double *params, int64_t nobs,
                                          const double *east, const double *north, double nu,
                                          double *out);

/* ---------------------------------------------------------------- PT proposal adaptation ---
 * replaces: the proposal update of every PT worker (sample_pt_chain, beat/sampler/pt.py:758-761; _iter_sample,
 *           beat/sampler/base.py:363-393; BaseChain.get_sample_covariance, beat/backend.py:249-268;
 *           calc_sample_covariance, beat/covariance.py:865-909: likelihood-weighted num.cov(..., aweights=, bias=False),
 *           then ensure_cov_psd).  The reference holds the window of buffer_size samples; here its weighted moments are
 *           accumulated on the device after every step, for G groups (temperatures) of R chains (replicas) at once.
 *
 *   state [G, 8 + n + n*n] doubles, group by group (a sub-range of groups is a sub-range of the array):
 *     [0] m       running maximum of `like` (-inf after reset)
 *     [1] S0      sum of w = exp(like - m)
 *     [2] Sw2     sum of w^2
 *     [3] count   rows accumulated
 *     [4] nbad    rows skipped because their like or state was not finite
 *     [5..7]      spare (0)
 *     [8 .. 8+n)  S1 = sum of w y,  y = x - ref
 *     [8+n ..)    S2 [n, n] = sum of w y y^T, lower triangle (entries above the diagonal stay 0)
 *
 *   _reset: the empty state; with ref [G, n] not NULL also ref[g] = mean of rows g*R .. g*R+R-1 of Q, summed in replica
 *     order (a window opens around the group's present states); Q, R unused otherwise.
 *   _update: rows g*R .. g*R+R-1 of Q [G*R, n] belong to group g; like[(g*R + r) * like_stride]; ref [G, n] the
 *     reference point of the group's window (constant while the window is open).  m' = max(m, max like), every
 *     accumulator is rescaled by exp(m - m') (Sw2 by its square) and the rows are added in replica order.  The sums
 *     of a group depend on (group, replica, order of the calls) alone -- not on G, on the other groups of the call or
 *     on where the arrays live.  G <= 64, R <= 1024, n <= 2048.
 *   _factor: mu = S1/S0, fact = 1 - Sw2/S0^2, cov = (S2/S0 - mu mu^T)/fact (symmetrised by copy) and its upper
 *     Cholesky factor F [G, n, n], F^T F = cov -- the `factor` of beatamd_proposal_draw.  flags [G]: 0 factored;
 *     1 fact <= 0, nbad > 0 or a non-finite value (the reference's cov = None: keep the previous proposal);
 *     2 not positive definite.  The factor of a flagged group is left untouched.  cov [G, n, n] (NULL: not wanted)
 *     is written for every group (the caller repairs a group flagged 2 with utility.ensure_cov_psd). */
int beatamd_group_moments_reset(beatamd_ctx *ctx, int64_t G, int64_t nparams, double *state, int64_t R, const double *Q,
                                double *ref);
int beatamd_group_moments_update(beatamd_ctx *ctx, int64_t G, int64_t R, int64_t nparams, const double *Q,
                                 const double *like, int64_t like_stride, const double *ref, double *state);
int beatamd_group_moments_factor(beatamd_ctx *ctx, int64_t G, int64_t nparams, const double *state, double *factor,
                                 double *cov, int32_t *flags);
/* beatamd_proposal_draw / beatamd_ffi_mstep_batch (multivariate) with one factor per group of chains (the proposals a
 * PT worker learned from its own trace, beat/sampler/pt.py:758-761): factor [G, K, nparams], chain c of the call draws
 * with factor c / (C / G); C must be a multiple of G.  Philox counters, df, the prior box, parking, the counters and
 * graph capture are those of the ungrouped entries; with G copies of one factor the results are bit for bit theirs. */
int beatamd_proposal_draw_grouped(beatamd_ctx *ctx, int64_t C, int64_t G, int64_t K, int64_t nparams,
                                  const double *factor, uint64_t seed, uint32_t step, int64_t first_chain, int32_t df,
                                  double *delta, double *log_u);
int beatamd_ffi_mstep_batch_grouped(beatamd_ctx *ctx, int32_t model_id, int64_t C, int64_t G, double *Q0, double *L0,
                                    const double *factor, int64_t K, int32_t df, uint64_t seed, uint32_t step,
                                    int64_t first_chain, const double *scaling, const double *lower,
                                    const double *upper, double beta, const double *betas, int32_t *accepted,
                                    int32_t *accepted_sum, int64_t *n_accepted);

/* replaces: DistributionOptimizer.lsq_solution(point)   beat/models/problems.py:753-873
 *           (the `initialization: lsq` start of an FFI run, beat/config.py:1121-1126, beat/models/base.py:216-231)
 * With the kinematics of a point fixed, the synthetics are linear in ONE inverted slip variable v (uparr or utens; the
 * reference's stacking of its blocks is shape-consistent for exactly one); a second sampled slip variable (uperp) is set
 * to zero.  The rows of the reference's design matrix A and right-hand side d, in this order:
 *   seismic    per wavemap, target t, sample n: A[(t,n), p] = the synthetic of patch p alone with unit slip
 *              (seismic.py:1351-1507 with patchidxs=[p]: the library row of v that the point's start time and duration
 *              select -- itself for nearest neighbour, the four-corner blend of ffi/base.py:663-709 for multilinear);
 *              d = the wavemap's data.  No weights, no hyper-parameters.
 *   geodetic   A = G_v^T [Nobs, P]; d = the displacements WITHOUT odw minus the dataset corrections at the point
 *              (apply_corrections(..., operation="-"), geodetic.py:411-427)
 *   laplacian  A = L h^2 with h = q[h_laplacian] as sampled (problems.py:845-848); d = 0
 * A is never formed.  Per chain the entries give the normal equations
 *     N_c = sum_wm sum_t R_ct R_ct^T + G_v G_v^T + h_c^4 L^T L        b_c = sum_wm sum_t R_ct d_t + G_v (d_geo - corr_c)
 * (R_ct [P, N]: the chain's rows for target t; G_v G_v^T and L^T L are formed once per model and kept until its data,
 * corrections or laplacian are replaced) and solve them under x >= 0 by Lawson & Hanson's active set, the algorithm of
 * scipy.optimize.nnls (problems.py:854).  Every sum has a fixed order that depends on the chain alone: the results of a
 * chain are bit for bit the same alone, in any batch and in any chunk.
 * set_lsq_variables: index (into the layout's slip variables) of the inverted variable and of the one set to zero (-1:
 *   none).  A model without a laplacian is BEATAMD_EINVAL with the reference's text (problems.py:768-772).
 * lsq_normal_batch: Q [C, nparams] -> N [C, P, P] (exactly symmetric), b [C, P]; chain_bad [C] (nullable): 1 for a chain
 *   whose times leave the library grid -- the call then fills the arrays and returns BEATAMD_EINDEX, as the likelihood
 *   flags such chains.
 * nnls_batch: N [C, n, n] (symmetric; n <= 1024), b [C, n] -> x [C, n], iters [C] (solves of the passive system, at
 *   least one per variable that enters), status [C]: 0 converged, 1 the cap of 3 n iterations reached (scipy raises
 *   RuntimeError("Maximum number of iterations reached.")), 2 non-finite N or b or a passive block that is not
 *   positive definite (x = NaN).  Tolerance on the dual: 10 n 2^-52 max|b|.  One wavefront per chain, the passive
 *   set's Cholesky factor in n^2 doubles of scratch per chain; batches run in chunks of chains whose scratch stays
 *   within 256 MiB.
 * lsq_solution_batch: both of the above, then Q_out = Q_in with v <- x and the zeroed variable <- 0.  The solution is
 *   NOT clipped to the prior box (the reference does not clip).  Chunks of chains keep the normal matrices within 1 GiB
 *   of scratch.  Q_in and Q_out may be the same array.  A flagged chain is BEATAMD_EINDEX. */
int beatamd_ffi_model_set_lsq_variables(beatamd_ctx *ctx, int32_t model_id, int32_t inverted, int32_t zeroed);
int beatamd_ffi_lsq_normal_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *N, double *b,
                                 int32_t *chain_bad);
int beatamd_nnls_batch(beatamd_ctx *ctx, int64_t C, int64_t n, const double *N, const double *b, double *x,
                       int32_t *iters, int32_t *status);
int beatamd_ffi_lsq_solution_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q_in, double *Q_out,
                                   int32_t *iters, int32_t *status);

/* ---- geodetic FFI library and resolution-based fault discretization (csrc/geolib.hip, csrc/resolution.hip)
 * Reference: geo_construct_gf_linear / geo_construct_gf_linear_patches (beat/ffi/base.py:804-1002),
 * get_smoothing_operator_correlated (beat/models/laplacian.py:261-298), optimize_discretization
 * (beat/ffi/fault.py:1520-1987; Atzori & Antonioli 2011, Atzori et al. 2019).  Array arguments may live on either side.
 * geo_gf_library: params [nrows, 10] (the slots of halfspace_displacements_batch: km, deg, m; rectangular sources, depth
 *   = top centre; the caller states rake / slip / opening of the slip component in each row, rows ordered
 *   (component, patch)); east, north [nobs] km; los [nobs, 3] = (Sn, Se, Su); odw [nobs] ->
 *   G [nrows, nobs] = (u_n S_n + u_e S_e + u_u S_u) * odw (base.py:813), every row in ONE launch.
 * smoothing_correlated: coords [P, 3] km, kind 0 "gaussian" 1/d^2 | 1 "exponential" 1/exp(d) -> L [P, P], the column
 *   sums taken over the rows in ascending order, the diagonal their negative.
 * model_resolution: gfs [P, nobs] (library rows = G^T), L [P, P] -> R [P, P] = inv(G^T G + eps^4 L^T L) . G^T G and
 *   diag [P] (fault.py:1805-1815).  A normal matrix that is not positive definite is BEATAMD_ENOTPSD.
 * division_rating: widths, lengths [P] km; centers [P, 3] km (event-relative east, north, depth); bottom_depth [P] m (of
 *   the patch's subfault); data_en [nobs, 2] km (east, north); mean_R [P] -> rating [P] = area * c1 * c2 * c3 and
 *   dmin [P] (nullable), the smallest horizontal distance of a patch centre to a data point (fault.py:1884-1929).  The
 *   argsort and the alpha cut stay with the caller. */
int beatamd_geo_gf_library(beatamd_ctx *ctx, int64_t nrows, const double *params, int64_t nobs, const double *east,
                           const double *north, const double *los, const double *odw, double nu, double *G);
int beatamd_smoothing_correlated(beatamd_ctx *ctx, int64_t P, const double *coords, int32_t kind, double *L);
int beatamd_model_resolution(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *gfs, const double *L,
                             double epsilon, double *R, double *diag);
int beatamd_division_rating(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *widths, const double *lengths,
                            const double *centers, const double *bottom_depth, double depth_penalty,
                            const double *data_en, const double *mean_R, double *rating, double *dmin);

/* ---- posterior marginals of a population or trace (csrc/marginals.hip, which states the orders the kernels promise)
 * replaces: the arrays behind `beat plot stage_posteriors`, `correlation_hist` and `lune`:
 *   histplot_op / hist_binning (beat/plotting/common.py:248-397: num.percentile at :303, :361), make_bins and traceplot
 *   (beat/plotting/marginals.py:131-507, :207-215), hist2d_plot_op (common.py:400-415), kde2plot_op (common.py:445-461)
 *   per variable pair of correlation_plot / correlation_plot_hist (marginals.py:510-609, 614-851), spherical_kde_op
 *   (common.py:471-523) with vonmises_fisher / vonmises_std (beat/models/distributions.py:245-337) for draw_lune_kde
 *   (beat/plotting/seismic.py:2707-2729).
 * X [n, V] row-major; cols [K] / pairs [P, 2]: column indices in [0, V) (BEATAMD_EINDEX outside), any order, repeats
 * allowed.  Array arguments may live on either side.  A non-finite sample in a used column is BEATAMD_ENAN, the message
 * and *bad_col (nullable) name the column (numpy would sort NaN last and return NaN).
 * column_sort: sorted [K, n] = the columns ascending (n <= 2^24).
 * column_percentiles: sorted [K, n], q [Q] in [0, 100] -> out [K, Q], bit for bit numpy.percentile's default ("linear").
 * column_histograms: edges [K, nb + 1], every row finite and non-decreasing -> counts [K, nb]: bin i counts
 *   edges[i] <= x < edges[i + 1], the last bin closed on the right (numpy.histogram).  Densities stay with the caller.
 * pair_hist2d: xedges [P, bx + 1], yedges [P, by + 1] -> counts [P, bx, by]: bin = searchsorted(edges, x, 'right') - 1,
 *   a value on the last edge in the last bin (numpy.histogram2d).  bx * by <= 128 * 128, each side <= 4096.
 * pair_kde2d: Z [P, gx, gy], Z[p, a, b] = scipy.stats.gaussian_kde of the pair's two columns (Scott's factor n^(-1/6),
 *   the sample covariance with bias=False, 1 / (2 pi n sqrt(det))) at (linspace(xmin, xmax, gx)[a],
 *   linspace(ymin, ymax, gy)[b]); extents [P, 4] = (xmin, xmax, ymin, ymax).  One accumulator per grid point, samples in
 *   ascending order: a Z does not depend on the other pairs of the call.  skip_blocks != 0 leaves out blocks of samples whose
 *   terms are exact zeros for a tile of the grid (the same bits).  shape: 0 lets the launcher choose between four grid
 *   points per lane in workgroups of 256 (1) and one per lane in workgroups of 64 (2, for few tiles); the same bits in
 *   both, here and in spherical_kde.  flags [P]: 1 for a pair whose scaled covariance has no
 *   Cholesky factor (a constant column, a column paired with itself, n < 3): its Z is NaN, the others hold their results
 *   and the call returns BEATAMD_ENOTPSD (scipy raises LinAlgError for such a pair).
 * unit_vector_sum: S [3] = sum_i (sin t cos p, sin t sin p, cos t), (t, p) = deg2rad of (lats, lons) (transform 0, the
 *   argument order and missing transform of vonmises_std's call in spherical_kde_op) or of (90 - lats, mod(lons, 360))
 *   (transform 1), summed in a fixed order.
 * spherical_kde: kde [m] = sum_i exp(norm + (x . x0_i) / sigma2) at the m points (lats, lons) over the n samples
 *   (lats0, lons0), all in degrees; norm = -log(4 pi sigma^2) - logsinh(1 / sigma^2) comes from the caller.  Samples are
 *   added in ascending order into one accumulator per point (the reference adds its remainder chunk first). */
int beatamd_column_sort(beatamd_ctx *ctx, int64_t n, int64_t V, const double *X, int64_t K, const int64_t *cols,
                        double *sorted, int64_t *bad_col);
int beatamd_column_percentiles(beatamd_ctx *ctx, int64_t K, int64_t n, const double *sorted, int64_t Q, const double *q,
                               double *out);
int beatamd_column_histograms(beatamd_ctx *ctx, int64_t K, int64_t n, const double *sorted, int64_t nb, const double *edges,
                              int64_t *counts);
int beatamd_pair_hist2d(beatamd_ctx *ctx, int64_t n, int64_t V, const double *X, int64_t P, const int64_t *pairs, int32_t bx,
                        int32_t by, const double *xedges, const double *yedges, int64_t *counts, int64_t *bad_col);
int beatamd_pair_kde2d(beatamd_ctx *ctx, int64_t n, int64_t V, const double *X, int64_t P, const int64_t *pairs, int32_t gx,
                       int32_t gy, int32_t skip_blocks, int32_t shape, double *Z, double *extents, int32_t *flags,
                       int64_t *bad_col);
int beatamd_unit_vector_sum(beatamd_ctx *ctx, int64_t n, const double *lats, const double *lons, int32_t transform, double *S);
int beatamd_spherical_kde(beatamd_ctx *ctx, int64_t n, const double *lats0, const double *lons0, int64_t m, const double *lats,
                          const double *lons, double norm, double sigma2, int32_t shape, double *kde);

/* ---- mechanism ensembles (csrc/mechanisms.hip; the per-draw arithmetic is csrc/mechanism.hpp's)
 * replaces: the arrays behind `beat plot fuzzy_beachball`, `fuzzy_mt_decomp` and `hudson`: the per-draw loop of mts2amps
 *   over lower_focalsphere_angles (beat/plotting/seismic.py:1334-1425), MomentTensor.standard_decomposition as
 *   fuzzy_mt_decomposition reads it (seismic.py:1664-1850, :1689-1696) and the (u, v) of draw_hudson (seismic.py:2183-2310).
 *   The decomposition and Hudson's projection restate pyrocko from memory and are pinned to multi-precision evaluations of
 *   the stated rules only (see mechanism.hpp).  Array arguments may live on either side.
 * mt_decompose: X [n, 6] = (mnn, mee, mdd, mne, mnd, med) (kind 0) or [n, 3] = strike, dip, rake in degrees (kind 1, the
 *   unit double couple of the polarity likelihood); n <= 2^24.  Outputs, each nullable: evals [n, 3] ascending and evecs
 *   [n, 3, 3] (columns) of the full tensor; moments, ratios [n, 5] and parts [n, 5, 6] in the order iso, dc, clvd, dev,
 *   full; unit [n, 5, 6], each part over sqrt(sum m9^2) / sqrt 2 (seismic.py:1410-1417; NaN for an all-zero part, as numpy
 *   gives); uv [n, 2], Hudson's (u, v).  A row with a non-finite entry or, kind 0, all six zero is BEATAMD_ENAN; the
 *   message names the first such row (numpy would spread NaN over the whole grid).
 * fuzzy_amps: unit [n, P, 6]; rw [6, npix], the propagation coefficients of the npix pixels inside the unit disc;
 *   pixel_index [npix], their cells iy * nx + ix in the (ny, nx) grid (BEATAMD_EINDEX outside), ny, nx <= 4096 -> amps
 *   [P, ny, nx]: NaN outside the pixels; mask != 0: the fraction of draws with a > 0, a = ((((r0 u0 + r1 u1) + r2 u2) +
 *   r3 u3) + r4 u4) + r5 u5 (seismic.py:1417-1423; integer counts, exact whatever the launch); mask == 0: sum of a over the
 *   draws in ascending order, one accumulator per pixel, over n.  shape as in pair_kde2d; the same bits in all three. */
int beatamd_mt_decompose(beatamd_ctx *ctx, int64_t n, int32_t kind, const double *X, double *evals, double *evecs,
                         double *moments, double *ratios, double *parts, double *unit, double *uv);
int beatamd_fuzzy_amps(beatamd_ctx *ctx, int64_t n, int32_t P, const double *unit, int64_t npix, const double *rw,
                       const int64_t *pixel_index, int32_t ny, int32_t nx, int32_t mask, int32_t shape, double *amps);

/* ---- producer of the seismic FFI Green's-function library (csrc/seislib.hip, which states the arithmetic contract)
 * replaces: seis_construct_gf_linear / _process_patch_seismic (beat/ffi/base.py:1005-1254) after the elementary
 *   waveforms: the convolution with the half-sinusoid source-time function of every duration (patch.stf.anchor = -1,
 *   base.py:1013), the filters of heart.Filter / BandstopFilter (beat/heart.py:366-412) and the taper, zero extension and
 *   [b, c] cut of post_process_trace / taper_filter_traces (beat/heart.py:3466-3525, 4242-4323), with
 *   ArrivalTaper.nsamples (beat/heart.py:295-304).  The waveforms themselves (pyrocko's engine.process) are the caller's.
 * Array arguments may live on either side.
 * stf_table: durations [D] >= 0 -> nt [D] = rint(duration / deltat) + 1 (each <= ntmax <= 65536, BEATAMD_EINVAL beyond)
 *   and A [D, ntmax], the normalised amplitudes (zero beyond nt; [1] for nt == 1).
 * trace_filter_batch: traces [R, L]; nt, A as stf_table wrote them (D = 1, ntmax = 1, nt = [1], A = [1]: no source-time
 *   function) -> Y [R, D, Lcmax], Lcmax = L + max(nt) - 1: row (r, d) holds the L + nt[d] - 1 samples of trace r convolved
 *   with row d of A and run through the cascade, zeros behind them.  The cascade: nstage <= 4 stages; ntaps [nstage] in
 *   [3, 17]; demean [nstage] (!= 0: the stage subtracts its input's mean first); coef [nstage, 2, 17] = b then a of every
 *   stage, a[0] = 1, entries beyond ntaps ignored.
 * seis_library_fill: responses [T, P, L]; i0, w0 [T, P, S]: first sample and the weight of sample 0 of every window ->
 *   lib [T, P, D, S, N]: lib[t, p, d, s, n] = Y[(t, p), d, i0 + n] inside the trace, 0 outside; sample 0 times w0.
 *   S, D <= 32767 (the library's int16 grid indices).  patch_block (<= 0: all P): the patches filtered at a time, which
 *   bounds the intermediate Y (T * patch_block * D * Lcmax doubles, allocated and freed by the call; BEATAMD_ENOMEM
 *   names the size).  The result does not depend on patch_block. */
int beatamd_stf_table(beatamd_ctx *ctx, int64_t D, const double *durations, double deltat, int64_t ntmax, int32_t *nt, double *A);
int beatamd_trace_filter_batch(beatamd_ctx *ctx, int64_t R, int64_t L, const double *traces, int64_t D, int64_t ntmax,
                               const int32_t *nt, const double *A, int32_t nstage, const int32_t *ntaps, const int32_t *demean,
                               const double *coef, double *Y);
int beatamd_seis_library_fill(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t L, const double *responses, int64_t D,
                              int64_t ntmax, const int32_t *nt, const double *A, int32_t nstage, const int32_t *ntaps,
                              const int32_t *demean, const double *coef, int64_t S, int64_t N, const int64_t *i0,
                              const double *w0, int64_t patch_block, double *lib);

/* ---- rupture fronts and polyline densities (csrc/rupture.hip, which states the orders the kernels promise)
 * replaces: the arrays behind `beat plot slip_dist`: the per-draw loop of fault.point2starttimes and matplotlib's
 *   ax.contour(xgr, ygr, sts) with automatic levels   fault_slip_distribution   beat/plotting/ffi.py:599-611, :645-648
 *   and the loop of draw_line_on_array over every contour line   fuzzy_rupture_fronts   beat/plotting/ffi.py:338-398
 *   (draw_line_on_array / _weighted_line beat/plotting/common.py:619-801, positions2idxs beat/utility.py:1556).
 *   The marching squares restate contourpy's "mpl2014" algorithm from its behaviour (a node is above iff z > level, a saddle
 *   is split by the mean of its corners, vertices by linear interpolation along the edge); the order of the lines and where a
 *   closed line starts are this library's own (see rupture.hip), not contourpy's.
 * sts [E, ncells_total]: the start times of E draws as they leave beatamd_ffi_start_times_batch; subs [nsub, 5] (int64) =
 *   (n_dip, n_strike, first patch, first x, first y) of every subfault, its patches row-major i * n_strike + j; x / y: the
 *   centre coordinates along strike / dip of all subfaults.  A subfault holds at most 2304 patches (BEATAMD_EINVAL above).
 * rupture_minmax: out [E, nsub, 2] = (min, max) of every (draw, subfault), both NaN where a start time is not finite.
 * contour_count: levels [E, nsub, 16], nlevels [E, nsub] (0 ... 16) -> counts [E, nsub, 16, 2] (int32) = (lines, vertices)
 *   of every level.  contour_fill: line_base / vert_base [E, nsub, 16] = the exclusive scans of those counts, nlines / nverts
 *   their totals -> vertices [nverts, 2] = (x, y) and line_offsets [nlines + 1] (entries 0 ... nlines - 1 are written; the last,
 *   nverts, is the caller's).  A closed line repeats its first vertex.  The output is a function of (draw, subfault, level,
 *   line, rank in the line) alone: bit for bit independent of how the draws are cut into calls.  Array arguments may live
 *   on either side.
 * polyline_density: grid [ny, nx] += the image of every selected polyline (sel [nsel] indices into the nlines lines, in
 *   drawing order; NULL: all, nsel == nlines), each drawn into an image of its own as beatamd_trace_density_update draws a
 *   trace -- the same cell indices, limits and arithmetic, the grid equals draw_line_on_array's called line by line bit
 *   for bit --; coverage [ny, nx] (int32, nullable) += 1 per polyline where its image is positive.  extent [4] = (xmin, xmax,
 *   ymin, ymax).  Errors as beatamd_trace_density_update: BEATAMD_EOUTSIDE for a vertex above the last cell or below
 *   -32768, BEATAMD_EINVAL for a vertex or extent that is not finite, ny, nx outside 2 ... 4096, linewidth outside (0, 64];
 *   BEATAMD_EINDEX for offsets or a selection outside their arrays. */
int beatamd_rupture_minmax(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int32_t nsub,
                           const int64_t *subs, double *out);
int beatamd_contour_count(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int32_t nsub,
                          const int64_t *subs, const double *levels, const int32_t *nlevels, int32_t *counts);
int beatamd_contour_fill(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int32_t nsub, const int64_t *subs,
                         int64_t nx_total, const double *x, int64_t ny_total, const double *y, const double *levels,
                         const int32_t *nlevels, const int64_t *line_base, const int64_t *vert_base, int64_t nlines,
                         int64_t nverts, double *vertices, int64_t *line_offsets);
int beatamd_polyline_density(beatamd_ctx *ctx, int64_t nverts, const double *vertices, int64_t nlines,
                             const int64_t *line_offsets, int64_t nsel, const int64_t *sel, const double *extent, int64_t ny,
                             int64_t nx, double linewidth, double *grid, int32_t *coverage);

/* ---- convergence summary of a trace (csrc/convergence.hip): the table ``beat summarize`` writes to summary.txt with
 * arviz.summary(idata, round_to=4, skipna=True) (apps/beat.py:1338-1363) from the result trace turned into inference data
 * (multitrace_to_inference_data, backend.py:1401-1415).  The statistics are restated from memory of arviz's
 * stats/diagnostics.py and of Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021), unverified against an installed arviz.
 * Arrays live on either side.
 * autocov_lags_batch (apps/beat.py:1338-1363, backend.py:1401-1415: the autocovariance behind every ESS): out [R, nlags],
 *   out[r, k] = (1/n) sum_i (y_i - m)(y_{i + lag0 + k} - m) of the R rows Y [R, n], m the row's mean, the biased estimate;
 *   a lag >= n gives 0.  Each lag is summed over ascending i in chunks of 4096 added in ascending order, one accumulator per
 *   lag: the value of a lag does not depend on lag0, nlags or R.
 * rank_normalize (apps/beat.py:1338-1363, backend.py:1401-1415: the transform of ess_bulk and r_hat): z [n] =
 *   normcdfinv((r - 3/8) / (n + 1/4)), r the average ranks (scipy.stats.rankdata "average"; -0.0 and 0.0 tie) of A [n], also
 *   written to ranks [n] where that is not NULL.  BEATAMD_ENAN for a non-finite value; n <= 2^24.
 * convergence_summary (apps/beat.py:1338-1363, backend.py:1401-1415): X [C, D, V] = C chains of D draws of V variables;
 *   out [K, 11] for the K columns cols = mean, sd, hdi_lo, hdi_hi, mcse_mean, mcse_sd, ess_bulk, ess_tail, r_hat, ess_mean,
 *   ess_sd.  The two mcse columns come back NaN: the caller forms them from sd, ess_mean and ess_sd.  hdi_prob in (0, 1).
 *   tau_floor = 1 / log10(2 C (D / 2)), the smallest autocorrelation time of an ESS, computed by the caller (<= 0: here).
 *   flags [K] = 1 for a column with a non-finite sample: its row is NaN (arviz's skipna would skip the sample).  D < 4: the
 *   diagnostics are NaN; mean, sd and the interval are filled.  var_batch > 0 fixes the variables of a pass over the
 *   workspace (0: sized to a budget), first_lags >= 2 the lags of the first round of the on-demand autocovariance (the next
 *   rounds take four times as many for the scans that have not stopped); neither changes a bit of out.  rounds (nullable):
 *   the largest number of rounds a pass took.  C D <= 2^24. */
int beatamd_autocov_lags_batch(beatamd_ctx *ctx, int64_t R, int64_t n, const double *Y, int64_t lag0, int64_t nlags, double *out);
int beatamd_rank_normalize(beatamd_ctx *ctx, int64_t n, const double *A, double *z, double *ranks);
int beatamd_convergence_summary(beatamd_ctx *ctx, int64_t C, int64_t D, int64_t V, const double *X, int64_t K,
                                const int64_t *cols, double hdi_prob, double tau_floor, int64_t var_batch, int64_t first_lags,
                                double *out, int32_t *flags, int64_t *rounds);

#ifdef __cplusplus
}
#endif
#endif /* BEAT_AMD_H */
