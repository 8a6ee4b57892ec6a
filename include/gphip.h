/*
 * gphip.h -- C ABI of libgphip.so: the MI355X-native (gfx950) exact-GP hot path.
 *
 * Drop-in boundary for the GPy / GPyOpt path named in BASELINE.json:north_star.
 * Each entry point cites the reference interface it replaces (paths relative
 * to the reference tree, file:line).  Plain pointers and sizes only; all
 * matrices are float64, C-contiguous (row-major), owned by the caller.  The
 * library copies host->device, owns all device memory inside the opaque
 * gp_t, writes results into caller-allocated buffers and keeps no host
 * pointer after returning.  One gp_t per device; calls are synchronous; a
 * gp_t is not thread-safe, distinct gp_t may be used from distinct threads
 * (gp_group_* below does exactly that for a single-threaded caller).
 *
 * Return codes: 0 = OK; k > 0 = leading minor k of Ky is not positive
 * definite even after the reference's jitter ladder (the host raises
 * numpy.linalg.LinAlgError with the reference's messages, GPy/GPy/util/
 * linalg.py:62-75); < 0 = bad argument / HIP / RCCL error (message via
 * gp_last_error()).  The library never aborts the process.
 */
#ifndef GPHIP_H
#define GPHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gp_ctx gp_t;

/* kernel families: GPy/GPy/kern/src/rbf.py:12-57 (RBF, alias ExpQuad), stationary.py:546-579 (Matern52),
 * stationary.py:447-482 (Matern32), stationary.py:384-392 (Exponential; OU :427-444 is the same covariance).
 * Out of scope: RatQuad (its `power` is a third hyper-parameter, which needs new outputs on gp_lml_grad, gp_fit_grad and
 * gp_fit_grad_batch); Cosine, kernel sums and products, active_dims; the Gower option with Matern32 / Exponential (the
 * fork gives Gower= / space= to RBF and Matern52 only). */
#define GP_KERNEL_RBF 0
#define GP_KERNEL_MATERN52 1
#define GP_KERNEL_MATERN32 2
#define GP_KERNEL_EXPONENTIAL 3

/* acquisitions: GPyOpt/GPyOpt/acquisitions/{EI,LCB,MPI}.py */
#define GP_ACQ_EI 0
#define GP_ACQ_LCB 1
#define GP_ACQ_MPI 2
/* or-ed into the `type` of a scoring entry: the scores are divided by the cost of the resident cost surface (the cost entries
 * near the end of this header).  Without it every entry behaves as it always did. */
#define GP_ACQ_PER_COST 0x100
/* black-box constraints (the feasibility entries at the end of this header).  GP_ACQ_TIMES_FEAS, or-ed into the `type` of the
 * entries named there, multiplies the scores by the cached probability of feasibility; GP_ACQ_POF is the rule whose value is 1
 * and whose gradient is 0 -- valid only together with GP_ACQ_TIMES_FEAS: the probability of feasibility alone, for the time
 * while no observation is feasible.  Without the flag every entry behaves as it always did. */
#define GP_ACQ_POF 3
#define GP_ACQ_TIMES_FEAS 0x200
#define GP_FEAS_MAX 8 /* constraints per call */
/* max-value entropy search (the gp_mes_* entries at the end of this header): the rule over the resident samples of the minimum's
 * value; `par` and `fmin` of a scoring call are ignored */
#define GP_ACQ_MES 4
#define GP_MES_MAX_K 64 /* samples of the minimum's value */
#define GP_MES_MAX_G 64 /* trial values per gp_mes_logsurv call */

/* error codes (< 0) */
#define GP_ERR_ARG (-1)
#define GP_ERR_HIP (-2)
#define GP_ERR_STATE (-3)
#define GP_ERR_RCCL (-4)
#define GP_ERR_NOT_PD_DIAG (-5) /* "not pd: non-positive diagonal elements", linalg.py:63-64 */

#define GP_TOPK_MAX 64 /* largest k of gp_acq_topk / gp_comm_allgather_topk */

/* ---- library / device -------------------------------------------------- */
const char *gp_last_error(void);
const char *gp_version(void);
int gp_device_count(int *count);
/* fills name (<= cap bytes), compute units, HBM bytes */
int gp_device_info(int device, char *name, int cap, int *cus, int64_t *hbm_bytes);

/* ---- lifetime ---------------------------------------------------------- */
/* Replaces constructing GPy.models.GPRegression / GP (GPy/GPy/models/gp_regression.py:29-36,
 * GPy/GPy/core/gp.py:38-110): an empty model bound to one device. */
int gp_create(gp_t **out, int device);
int gp_destroy(gp_t *gp);
/* Ordered library shutdown: waits for every device the library used, destroys the events of the live contexts and then
 * the per-device stream set (which otherwise lives for the whole process: hardware queues keep their command-processor
 * pipe only while they are never re-created).  Registered with atexit() at the first gp_create, so a process that
 * simply exits -- also under rocprofv3 -- tears the queues down before the HIP runtime's own exit handlers run.
 * Contexts still alive afterwards only accept gp_destroy. */
int gp_shutdown(void);

/* GP.set_XY (GPy/GPy/core/gp.py:202-238): X[N,D], Y[N,P] row-major, copied H2D. 1 <= P <= 128. */
int gp_set_data(gp_t *gp, const double *X, const double *Y, int64_t N, int D, int P);

/* Kernel + Gaussian-noise hyper-parameters in natural space
 * (Stationary.__init__ stationary.py:61-82; Gaussian variance likelihoods/gaussian.py:43).
 * kernel is one of GP_KERNEL_RBF, _MATERN52, _MATERN32, _EXPONENTIAL; any other id is GP_ERR_ARG, and so is _MATERN32 or
 * _EXPONENTIAL while the Gower option is on (gp_set_gower refuses likewise when it comes second).
 * lengthscale has 1 entry (ard = 0) or D entries (ard = 1). */
int gp_set_params(gp_t *gp, int kernel, int ard, double variance, const double *lengthscale, double noise);

/* The fork's mixed-variable "Gower" covariance (GPy/GPy/kern/src/stationary.py:116-135 of the reference tree):
 * K = prod_d K_of_r(r_d), r_d = |x_d - x'_d| / range[d] on continuous dimensions and (x_d != x'_d) on discrete
 * ones (is_discrete[d] != 0).  enable = 0 restores the Euclidean kernel.  Kdiag remains `variance`, as in the fork.
 * Predictive gradients of a Gower model (gp_predict_grad, gp_acq_grad, gp_acq_lp_grad) are the fork's: Euclidean
 * Stationary.gradients_X on the kernel's own lengthscale (stationary.py:336-364, _inv_dist :251-258) with the Gower
 * K(Xs, X) inside dv/dx (gp.py:451-452) -- what run.py:1206-1225,1244 runs L-BFGS and estimate_L on.  gp_lml_grad and
 * gp_fit_grad likewise return what the fork's update_gradients_full computes (stationary.py:218-238): the Gower K as the
 * weight of the variance gradient, Euclidean dK/dr on the kernel's own lengthscale in the lengthscale gradients.  Those
 * are NOT derivatives of the Gower model's LML (K does not depend on that lengthscale at all, and depends on the variance
 * as variance^D); the host layer derives the true gradient from them (D x the variance entry, 0 for the lengthscale) unless
 * told to follow the fork (GPRegression.gower_gradients). */
int gp_set_gower(gp_t *gp, int enable, const int *is_discrete, const double *range);

/* ---- fit ---------------------------------------------------------------
 * ExactGaussianInference.inference (GPy/GPy/inference/latent_function_inference/
 * exact_gaussian_inference.py:37-74) minus the gradient terms:
 *   K = kern.K(X) (stationary.py:107-193); Ky = K + (noise + 1e-8) I (:55-56);
 *   L = jitchol(Ky, maxtries) with the reference's jitter ladder (linalg.py:56-81);
 *   logdet = 2 sum log L_ii (linalg.py:208); alpha = Ky^-1 Y (dpotrs, :60);
 *   lml = 0.5 (-N P log 2pi - P logdet - sum(alpha * Y)) (:62).
 * Outputs: *lml, *logdet, *jitter_used (0 when the first dpotrf succeeds). */
int gp_fit(gp_t *gp, int maxtries, double *lml, double *logdet, double *jitter_used);

/* lml / logdet / jitter of the last fit (or of the root's fit after gp_comm_bcast_fit). */
int gp_get_fit_state(gp_t *gp, double *lml, double *logdet, double *jitter);
/* Posterior.woodbury_vector (posterior.py:198-214): alpha[N,P]. */
int gp_get_alpha(gp_t *gp, double *alpha);
/* Posterior.woodbury_chol: L[N,N] row-major, lower triangle (upper written as 0). */
int gp_get_chol(gp_t *gp, double *L);
/* Posterior.woodbury_inv (posterior.py:176-196): Ky^-1 [N,N], symmetric.  Computed lazily (potri). */
int gp_get_woodbury_inv(gp_t *gp, double *Wi);
/* kern.K(X) without noise (stationary.py:107-140), for parity tests of the K-build kernel: K[N,N]. */
int gp_kernel_matrix(gp_t *gp, double *K);
/* kern.K(X, X2) -- the cross covariance of the kernel contract (Kern.K, GPy/GPy/kern/src/kern.py:119;
 * Stationary.K with X2 given, stationary.py:107-140: _unscaled_dist's X2 branch :168-173 has no diagonal fix, the Gower
 * branch :116-135 likewise takes X2).  X = the training inputs of gp_set_data, X2[M2, D] row-major (caller-owned);
 * K[N, M2] row-major.  Uses the current kernel parameters; leaves the fit and the resident candidates untouched. */
int gp_cross_kernel_matrix(gp_t *gp, const double *X2, int64_t M2, double *K);

/* GP.parameters_changed gradient push-down (gp.py:268-269):
 *   dL_dK = 0.5 (alpha alpha^T - P Ky^-1) (exact_gaussian_inference.py:70);
 *   dnoise = sum diag(dL_dK) (gaussian.py:78-79);
 *   dvariance, dlengthscale[1 or D] = Stationary.update_gradients_full (stationary.py:218-238).
 * Natural-space gradients of the LML; the Logexp chain rule stays on the host. Requires gp_fit.
 * Limits (GP_ERR_ARG, nothing is launched and the context is left as it was): P <= 16 (GP_GRAD_MAX_P), and D and P JOINTLY --
 * the fused pass stages both 128-row tiles of the inputs (twice over for a Gower model) and of alpha in LDS,
 *   576 + 2048 ((Gower ? 2 : 1) D + P) bytes a workgroup,
 * which must fit what the device gives a workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock, read in gp_create).  On gfx950
 * (163840 bytes): D + P <= 79, for a Gower model 2 D + P <= 79 -- D = 64 with P = 16 is refused, and a Gower model of D >= 40
 * has no gradient entry.  The message names D, P, the Gower setting, the bytes needed and the bytes there are.  The same limit
 * holds for gp_fit_grad, gp_fit_grad_x, gp_fit_grad_warp and the three batch entries below, checked before their factorisation;
 * gp_lml_grad_x (2048 (D + P) bytes) and gp_sparse_fit_grad (1024 (2 D + P)) fit at every accepted shape there and are checked
 * all the same. */
int gp_lml_grad(gp_t *gp, double *dvariance, double *dlengthscale, double *dnoise);
/* The two sides of that comparison for the context's data and Gower setting: *need bytes of LDS a workgroup of the gradient
 * pass, *available bytes the device gives one.  Requires gp_set_data (GP_ERR_STATE). */
int gp_lml_grad_lds(gp_t *gp, int64_t *need, int64_t *available);

/* grad_dict['dL_dK'] of ExactGaussianInference.inference (exact_gaussian_inference.py:70,74):
 *   dL_dK[N,N] = 0.5 (alpha alpha^T - P Ky^-1), the matrix GP.parameters_changed hands to
 *   kern.update_gradients_full (gp.py:269) -- for reference-side kernels that reduce it on the host.
 *   (gp_lml_grad reduces the same matrix on the device without materialising it.)  Requires gp_fit. */
int gp_get_dl_dk(gp_t *gp, double *dL_dK);

/* gp_fit + gp_lml_grad as ONE call -- what every L-BFGS evaluation of the hyper-parameter loop asks for
 * (Model.objective_function + objective_function_gradients, GPy/GPy/core/model.py:96-127; GPyOpt
 * models/gpmodel.py:88-93).  The first "pipe_stages_grad" stages of the solve for L^-T (dpotri, linalg.py:127-145)
 * ride behind the factorisation's latency-bound tail.  Same results as the two calls in sequence. */
int gp_fit_grad(gp_t *gp, int maxtries, double *lml, double *logdet, double *jitter_used, double *dvariance,
                double *dlengthscale, double *dnoise);

/* InputWarpedGP.parameters_changed (GPy/GPy/models/input_warped_gp.py:94-103): kern.gradients_X(dL_dK, X) with X2 = None,
 * Stationary.gradients_X (stationary.py:336-352 with tmp + tmp.T, _inv_dist :251-258) -- the LML's gradient with respect to the
 * training inputs, which the warping function's update_grads turns into gradients of its parameters:
 *   dL_dX[i, q] = (1 / l_q^2) sum_{j != i} 2 dL_dK_ij g(r_ij) (x_iq - x_jq),  g(r) = dK_dr(r) / r, 0 at r = 0
 * dL_dX[N, D] row-major.  One pass over Ky^-1 per 16 dimensions (csrc/gradx.hip), no atomics: the same bits from run to run.
 * Always true fp64; under "emulate_fp64" it reads whichever Ky^-1 the fit produced.  Requires gp_fit (GP_ERR_STATE); P <= 16
 * and no Gower model (the fork's Euclidean gradients_X on a Gower K is not a derivative of anything), else GP_ERR_ARG.
 * Leaves the fit, the validity flags and the resident candidates as gp_lml_grad leaves them. */
int gp_lml_grad_x(gp_t *gp, double *dL_dX);

/* gp_fit_grad followed by gp_lml_grad_x as ONE call with one final hand-over: what every L-BFGS evaluation of the
 * input-warped model asks for (the warped inputs moved, so gp_set_data precedes it).  The first eight outputs are bitwise
 * those of gp_fit_grad, dL_dX[N, D] bitwise that of gp_lml_grad_x after it.  Return codes as gp_fit_grad and gp_lml_grad_x. */
int gp_fit_grad_x(gp_t *gp, int maxtries, double *lml, double *logdet, double *jitter_used, double *dvariance,
                  double *dlengthscale, double *dnoise, double *dL_dX);

/* gp_fit_grad for R parameter vectors over the resident (X, Y) in ONE call: member r has variance[r], lengthscale[r*nls ...]
 * (nls = 1, or D with ard, from the last gp_set_params) and noise[r]; kernel, ard and the Gower set-up are the context's.
 * Replaces the serial restarts of GPModel.updateModel (GPyOpt/GPyOpt/models/gpmodel.py:78-93: optimize_restarts of
 * GPy/GPy/core/model.py:96-127 evaluations) with restarts in lockstep, one call per round of L-BFGS steps.  Member r runs the
 * single-stream route of gp_fit_grad (jitter ladder of linalg.py:62-75 per member: only failed members are factored again)
 * with the member as a batch index of every launch.  status[r] = 0, or what gp_fit_grad returns for that member (its outputs
 * are then NaN); a failed member does not fail the call.  Npad <= 2048 and 1 <= R <= 64, else GP_ERR_ARG; positive
 * parameters.  Always true fp64 ("emulate_fp64" does not apply).  The resident fit (L, alpha, Ky^-1, parameters, fitted /
 * predicted state) is untouched: the batch has buffers of its own, allocated at first use, about 5 Npad^2 doubles per member. */
int gp_fit_grad_batch(gp_t *gp, int R, const double *variance, const double *lengthscale, const double *noise, int maxtries,
                      double *lml, double *logdet, double *jitter_used, double *dvariance, double *dlengthscale, double *dnoise,
                      int *status);

/* gp_fit_grad_x for R members in ONE call, member r over inputs of its own, Xw[r] ([R, N, D] row-major, already warped by the
 * caller); Y, kernel family, ard are the context's, the parameters per member as in the plain batch entry.  dL_dX is [R, N, D].
 * What InputWarpedGP's restarts in lockstep ask for (GPy/GPy/models/input_warped_gp.py:94-103 per member): each member's warp
 * parameters differ, so its training inputs do.  The contract is the plain batch entry's -- 1 <= R <= 64, Npad <= 2048,
 * positive parameters, the jitter ladder per member, status[r] with NaN outputs (the member's dL_dX block included) for a member
 * that fails, always true fp64, buffers of the batch's own -- plus gp_lml_grad_x's refusals: the Gower option on, P > 16
 * (GP_ERR_ARG).  Xw travels in one copy (R N D doubles, at most 64 x 2048 x 64).  The resident fit, X, Y, raw targets, output
 * warp and its log-Jacobian, candidates and every validity flag are untouched; with an output warp on, the members fit the
 * warped targets the context holds.  Where Npad <= 768 member r's outputs are bitwise those of gp_set_data(Xw[r], Y) +
 * gp_fit_grad_x with its parameters (the single call takes the single-stream route the batch mirrors); above, they agree to
 * rounding. */
int gp_fit_grad_x_batch(gp_t *gp, int R, const double *Xw, const double *variance, const double *lengthscale,
                        const double *noise, int maxtries, double *lml, double *logdet, double *jitter_used, double *dvariance,
                        double *dlengthscale, double *dnoise, double *dL_dX, int *status);

/* ---- predict -----------------------------------------------------------
 * Candidates Xs[M,D] are made resident once; the calls below then run on them. */
int gp_set_candidates(gp_t *gp, const double *Xs, int64_t M);

/* gp_set_candidates(w(Xs)) for the input-warped GP: KumarWarping.f (GPy/GPy/util/input_warping_functions.py:179-200) applied
 * to the table on the device.  The un-warped Xs[M, D] goes host-to-device as in gp_set_candidates; one elementwise kernel
 * (csrc/gradx.hip) then overwrites the resident block, "mc_max" rows per launch:
 *   column q with warp[q] != 0:  1 - (1 - u^a[q])^b[q],  u = (x - xmin[q]) / (xmax[q] - xmin[q])   (double-precision pow;
 *                                u outside [0, 1] gives what NumPy's power gives the reference, NaN for fractional exponents)
 *   column q with warp[q] == 0:  the value itself, bit for bit.
 * warp, a, b, xmin, xmax have D entries each (a, b, xmin, xmax are read only where warp[q] is set); the caller passes xmin /
 * xmax already widened by its epsilon.  warped_out[M, D], when not NULL, receives the warped table.  a or b non-positive or
 * non-finite, or xmax <= xmin, is GP_ERR_ARG.  No state is kept: nothing else in the context learns of the warp. */
int gp_set_candidates_kumar(gp_t *gp, const double *Xs, int64_t M, const int *warp, const double *a, const double *b,
                            const double *xmin, const double *xmax, double *warped_out);

/* PosteriorExact._raw_predict (posterior.py:273-302, full_cov = False) followed by
 * Gaussian.predictive_values (likelihoods/gaussian.py:102-110) when include_noise != 0:
 *   mean[M,P] = K(Xs,X) alpha;  var[M] = variance - sum_rows (L^-1 K(X,Xs))^2 (+ noise).  No clipping. */
int gp_predict(gp_t *gp, int include_noise, double *mean, double *var);

/* gp_fit + gp_predict on the resident candidates as ONE call.  The first "pipe_stages" (3 at N = 16384) panel stages of
 * the candidate solve ride behind the factorisation once "pipe_start_pct" % (default: 32 up to 24 panels, 40 beyond) of its panels are done --
 * from there the factorisation's latency chain leaves CUs idle -- and the rest run after it.  Bitwise the results of
 * the two calls in sequence; 5 % faster at N=16384, M=10^4 (BO.suggest_next_locations always runs the two back to
 * back: GPyOpt/GPyOpt/core/bo.py:236-254 then acquisitions/base.py:33-39). */
int gp_fit_predict(gp_t *gp, int maxtries, int include_noise, double *lml, double *logdet, double *jitter_used,
                   double *mean, double *var);

/* full_cov = True branch (posterior.py:280-284): cov[M,M] = K(Xs) - tmp^T tmp (+ noise I). */
int gp_predict_full_cov(gp_t *gp, int include_noise, double *mean, double *cov);

/* GP.posterior_samples_f (gp.py:581-609) on the resident candidates: the full posterior covariance
 * (posterior.py:280-284, + noise I when include_noise) is factored on the device, C C^T = cov, under GPy's jitter
 * ladder (jitchol, linalg.py:56-81; maxtries as there), and applied to the caller's standard normals Z[S,M]:
 *   dev[S,M] = (C z_s)^T;  a draw of output d is mean[:,d] + dev[s,:].  mean[M,P] may be NULL.
 * M <= "mc_max".  Return codes as gp_fit (k > 0: not positive definite even with jitter). */
int gp_posterior_samples(gp_t *gp, int include_noise, const double *Z, int S, int maxtries, double *mean, double *dev,
                         double *jitter_used);

/* GP.predictive_gradients (gp.py:407-454): dmdx[M,D,P], dvdx[M,D].  dvdx = NULL: the mean's gradients alone
 * (gradients_X(alpha^T, X*, X), gp.py:433-438) -- what estimate_L maximises over 500 + N points
 * (GPyOpt/GPyOpt/core/evaluators/batch_local_penalization.py:55-64); they need neither Ky^-1 nor K(X*, X) Ky^-1. */
int gp_predict_grad(gp_t *gp, double *dmdx, double *dvdx);

/* GPModel.get_fmin (GPyOpt/GPyOpt/models/gpmodel.py:125-129): min over the training
 * inputs of the posterior mean.  Cached per fit (the reference recomputes it per call).  Under an output warp it stays
 * in latent space: the minimum of the mean of f(Y). */
int gp_fmin(gp_t *gp, double *fmin);

/* AcquisitionBase.acquisition_function on the resident candidates
 * (GPyOpt/GPyOpt/acquisitions/base.py:33-39 with constant cost and no constraints):
 * GPModel.predict (gpmodel.py:95-112: var clipped at 1e-10, s = sqrt(v), with noise),
 * get_quantiles (util/general.py:113-129), EI.py:32-40 / LCB.py:31-37 / MPI.py:32-40.
 * par = jitter (EI, MPI) or exploration weight (LCB).  Requires P == 1.
 * y_mean / y_std undo a host-side Standardize normalizer (1 / 0 when none).
 * out[M] holds the NEGATED acquisition, as the reference returns it. */
int gp_acq(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, double *out);

/* Same scores reduced on the device: sense = +1 -> argmax of out, -1 -> argmin of out
 * (run.py:1240-1241 takes argmax; anchor_points_generator.py:61 takes the smallest);
 * ties resolve to the lowest index (NumPy argmax/argmin). idx is relative to this gp's
 * candidate set. */
int gp_acq_argbest(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std,
                   int sense, int64_t *idx, double *val);

/* The k best scores in order (AnchorPointsGenerator.get, GPyOpt/GPyOpt/optimization/anchor_points_generator.py:59-61:
 * argsort(scores)[:num_anchor]): idx[k], val[k]; equal scores come out lowest index first; when M < k the tail is
 * idx = -1.  1 <= k <= GP_TOPK_MAX. */
int gp_acq_topk(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int sense, int k,
                int64_t *idx, double *val);

/* acquisition_function_withGradients (base.py:42-50; EI.py:42-51, LCB.py:39-46, MPI.py:42-51):
 * out[M] negated value, dout[M,D] negated gradient. */
int gp_acq_grad(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std,
                double *out, double *dout);

/* Local-penalisation batch acquisition on the resident candidates (the evaluator run.py:1219,1238-1257 uses):
 * AcquisitionLP._penalized_acquisition (GPyOpt/GPyOpt/acquisitions/LP.py:70-89):
 *   out = -T(acq(x)) - sum_k log Phi((|x - Xb_k| - r_x0[k]) / s_x0[k]),  T = log(. + 1e-50) (transform 0) or
 *   log(softplus(.)) (transform 1); acq is the base EI / LCB / MPI value; r_x0, s_x0 from
 *   _hammer_function_precompute (LP.py:49-62), computed by the host from gp_predict at the batch points.
 * nb = 0 gives the un-penalised log acquisition.  out[M] as the reference returns it (to be minimised). */
int gp_acq_lp(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int transform,
              const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out);
/* AcquisitionLP.acquisition_function_withGradients (LP.py:112-140) on the resident candidates: out[M] as gp_acq_lp,
 * dout[M,D] = scale * d(-acq)/dx - sum_k pen_k, with scale = 1 / acq (transform 0) or 1 / (softplus(acq) (1 + exp(-acq)))
 * (transform 1) and pen_k = exp(-z^2/2) / (s_x0[k] sqrt(2 pi) Phi(z) |x - Xb_k|), z = (|x - Xb_k| - r_x0[k]) / s_x0[k],
 * taken as 0 where Phi(z) < 1e-50.  The reference's _d_hammer_function (LP.py:91-103) sums that SCALAR over the batch and
 * subtracts it from every input dimension (the direction (x - Xb_k) / |x - Xb_k| is missing there); reproduced as is so that
 * an L-BFGS run over this function follows the reference's. */
int gp_acq_lp_grad(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int transform,
                   const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out, double *dout);
/* arg-best of the same vector, skipping the rows listed in exclude (run.py:1249-1252). */
int gp_acq_lp_argbest(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int transform,
                      const double *Xb, int nb, const double *r_x0, const double *s_x0, int sense,
                      const int64_t *exclude, int nex, int64_t *idx, double *val);

/* ---- output-warped GP ----------------------------------------------------------------------------------------------------
 * GPy.models.WarpedGP (GPy/GPy/models/warped_gp.py:13-160) behind GPyOpt's WarpedGPModel (GPyOpt/GPyOpt/models/
 * warpedgpmodel.py:15-68): the GP is fitted to f(Y), f the monotone warp of Snelson et al. (TanhFunction,
 * GPy/GPy/util/warping_functions.py:71-169)
 *   f(y) = d y + sum_i a_i tanh(b_i (y + c_i)),  i < n_terms <= 8,
 * with psi[3 n_terms] = (a_0, b_0, c_0, a_1, ...) row-major as the reference's psi matrix.  Valid parameters are finite with
 * a_i >= 0, b_i >= 0 and d > 0 (f is then strictly increasing); anything else, or n_terms outside 0..8, is GP_ERR_ARG.  The
 * warp's arithmetic is csrc/warp_math.h, its kernels csrc/warp.hip; every reduction has a fixed order, so the same input
 * gives the same bits on every call.
 *
 * While a warp is on, the fit, its gradients, the posterior and the acquisition entry points work in LATENT space, on f(Y):
 * so does the cached minimum of the training mean (the fmin entry point).  The plain batched fit-and-gradient returns GP_ERR_STATE
 * (its members share Y, and each would need targets warped by parameters of its own: that is the warp batch entry below, whose
 * members each warp the raw targets), and so do the group entry points that
 * load, fit or score (a group replicates one un-warped model). */

/* WarpedGP.transform_data + the Jacobian term of log_likelihood (warped_gp.py:42,47-57): the resident targets become
 * f(Y_raw), *log_jacobian = sum_n log f'(y_n) -- what the host adds to the LML.  The raw targets are kept in a buffer of
 * the context's own, so the call may be repeated with other parameters; n_terms = 0 switches the warp off and restores
 * the raw targets (psi may be NULL, d is ignored, *log_jacobian = 0).  Needs data with P = 1 (GP_ERR_STATE otherwise);
 * drops the fit.  A later upload of data with P = 1 warps the new targets with the parameters in force; with P != 1 it is
 * refused (GP_ERR_STATE) until the warp is off. */
int gp_set_output_warp(gp_t *gp, int n_terms, const double *psi, double d, double *log_jacobian);

/* The resident targets as the fit sees them, Y[N, P]: the caller's own without a warp, f(Y_raw) under one -- WarpedGP's
 * Y_normalized after transform_data (warped_gp.py:42). */
int gp_get_targets(gp_t *gp, double *Y);

/* TanhFunction.update_grads (warping_functions.py:159-169) with Kiy the resident alpha (warped_gp.py:44-45): natural-space
 * gradients of LML + log-Jacobian with respect to the warp's parameters,
 *   grad_psi = -sum_n alpha_n df/dpsi(y_n) + sum_n (df'/dpsi)(y_n) / f'(y_n),
 * dpsi[3 n_terms] laid out as psi, *dd for d.  Requires a fit and an active warp (GP_ERR_STATE). */
int gp_warp_grad(gp_t *gp, double *dpsi, double *dd);

/* The three steps of one L-BFGS evaluation of the warped model (WarpedGP.parameters_changed, warped_gp.py:38-45) as ONE call:
 * the warp of the targets with the new parameters, the fit with its hyper-gradients, the warp's gradients.  Outputs are
 * bitwise those of the three calls in sequence; return codes theirs.  1 <= n_terms <= 8. */
int gp_fit_grad_warp(gp_t *gp, int n_terms, const double *psi, double d, int maxtries, double *lml, double *logdet,
                     double *jitter_used, double *dvariance, double *dlengthscale, double *dnoise, double *log_jacobian,
                     double *dpsi, double *dd);

/* gp_fit_grad_warp for R members in ONE call (WarpedGP's restarts in lockstep): member r fits f_r(Y_raw), f_r the tanh warp
 * psi[r] ([R, n_terms, 3]), d[r], of the context's RAW targets (those of gp_set_data, whether or not a warp is on), with
 * kernel parameters of its own as in the plain batch entry.  log_jacobian[R], dpsi[R, n_terms, 3], dd[R] are the member's
 * sum log f_r', and the gradients gp_warp_grad gives.  The contract is the plain batch entry's -- 1 <= R <= 64, Npad <= 2048,
 * positive kernel parameters, the jitter ladder per member, status[r] with NaN outputs (log_jacobian, dpsi and dd included) for
 * a member that fails, always true fp64 -- plus: P = 1, 1 <= n_terms <= 8 and valid warp parameters for every member, else
 * GP_ERR_ARG.  The resident fit, X, Y, raw targets, the warp in force and its log-Jacobian, candidates and every validity flag
 * are untouched: the members' targets live in the batch's own buffers.  Bitwise gp_fit_grad_warp per member where Npad <= 768. */
int gp_fit_grad_warp_batch(gp_t *gp, int R, int n_terms, const double *psi, const double *d, const double *variance,
                           const double *lengthscale, const double *noise, int maxtries, double *lml, double *logdet,
                           double *jitter_used, double *dvariance, double *dlengthscale, double *dnoise, double *log_jacobian,
                           double *dpsi, double *dd, int *status);

/* WarpedGP.predict with predict_in_warped_space (warped_gp.py:62-116) over the resident candidates: the latent posterior
 * (computed first unless the resident one is current), un-normalised as mean y_std + y_mean, var y_std^2 BEFORE the warp is
 * inverted (warped_gp.py:101), is pushed through f^-1 at the deg <= 64 Gauss-Hermite nodes[deg] / weights[deg] the caller
 * supplies (numpy.polynomial.hermite.hermgauss):
 *   y_k = f^-1(m + sqrt2 sigma t_k);  mean[M] = sum w_k y_k / sqrt(pi);  var[M] = sum w_k y_k^2 / sqrt(pi) - mean^2.
 * want_median != 0: median[M] = f^-1(m) as well.  partials[M, 4], when not NULL: (d mean / d m, d mean / d sigma,
 * d var / d m, d var / d sigma) of the un-normalised m and sigma.  A candidate's numbers depend on its own (m, sigma) only,
 * not on M or its row.  Deviations from the reference: sigma = sqrt(max(var, 0)) (the reference takes the root of a negative
 * variance and returns NaN); f^-1 is a Newton iteration kept inside the bracket [(z - sum a) / d, (z + sum a) / d] and run to
 * a step below 2^-52 max(1, |y|), not the reference's 250 damped sweeps with their stopping rule over the whole array
 * (warping_functions.py:34-57), which are still far from the root for steep warps.  With the warp off f is the identity.
 * Needs P = 1 (GP_ERR_STATE). */
int gp_predict_warped(gp_t *gp, int include_noise, double y_mean, double y_std, int deg, const double *nodes,
                      const double *weights, int want_median, double *mean, double *var, double *median, double *partials);

/* The same moments for a latent posterior given by value, mean_in[M] / var_in[M]: the route of a handful of locations after
 * the few-rows predict.  Bitwise what the resident route returns for the same (mean, var). */
int gp_warp_moments(gp_t *gp, const double *mean_in, const double *var_in, int64_t M, double y_mean, double y_std, int deg,
                    const double *nodes, const double *weights, int want_median, double *mean, double *var, double *median,
                    double *partials);

/* y[n] = f^-1(z[n]) with the warp in force: WarpedGP.predict_quantiles (warped_gp.py:118-132). */
int gp_warp_inverse(gp_t *gp, const double *z, int64_t n, double *y);

/* ---- a handful of locations per call: the acquisition optimiser's inner loop --------------------------------
 * scipy's L-BFGS-B evaluates the acquisition ONE location per call, hundreds of times between two fits
 * (GPyOpt/GPyOpt/optimization/optimizer.py:36-61 -> acquisitions/base.py:33-50, LP.py:105-140 -> models/gpmodel.py:95-142
 * -> GPy/GPy/core/gp.py:297-354,407-454).  These two entry points are gp_set_candidates followed by the batched calls
 * named below, as ONE call taking the locations Xs[M, D] by value; for M <= option "small_m" (8) locations of a
 * single-output model with min(M, 4) D <= 128 they run as three launches (two for a value-only call) per pass over the
 * explicit inverse factor L^-1 (dtrtri, linalg.py:217-227; built once per fit -- at the first call for N <= 4096, above
 * that after the first N / 768 calls, which go through substitutions against L: option "rows_build" -- at half the work of
 * Ky^-1) with no copy commands (csrc/onerow.hip), otherwise through the batched calls themselves.  A pass takes up to four
 * locations; 5 .. 8 locations with M D <= 128 are ONE wide pass (option "rows_wide", default 1), otherwise -- and with
 * "rows_wide" = 0 -- passes of four.  A location's results are the same bits whatever its slot, its company and the kind of
 * its pass.  Fused path and batched calls give the same results to rounding (tests/test_gpu_rows.py: 1e-9 on
 * well-conditioned models, the north-star 1e-6 against the oracle everywhere); the
 * resident candidate block of gp_set_candidates is unspecified afterwards.
 *
 * gp_predict_rows = gp_predict(include_noise, mean[M], var[M]) and, when dmdx / dvdx are given,
 *                   gp_predict_grad(dmdx[M, D], dvdx[M, D]).  mean / var may be NULL.  P = 1 layouts.  dmdx alone (dvdx,
 *                   mean, var NULL) = gp_predict_grad(dmdx, NULL): the mean's gradient, one pass over the training points
 *                   with no inverse factor behind it -- estimate_L's inner call (batch_local_penalization.py:55-67).
 * gp_acq_rows     = gp_acq / gp_acq_grad (lp = 0) or gp_acq_lp / gp_acq_lp_grad (lp = 1, with transform, Xb, nb, r_x0,
 *                   s_x0 as there): out[M], and dout[M, D] when given. */
int gp_predict_rows(gp_t *gp, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                    double *dvdx);
int gp_acq_rows(gp_t *gp, const double *Xs, int64_t M, int type, double par, double fmin, double y_mean, double y_std,
                int lp, int transform, const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out,
                double *dout);
/* how many of those calls took the fused path / the batched calls since gp_create (route checks of the tests) */
int gp_rows_stats(gp_t *gp, int64_t *fused, int64_t *fallback);
/* how many passes of at most four locations / wide passes (5 .. 8 locations) the fused path has made since gp_create */
int gp_rows_pass_stats(gp_t *gp, int64_t *narrow, int64_t *wide);

/* ---- appending observations ------------------------------------------------------------------------------------------
 * Append k rows to the data of a valid fit and extend the fit to them without refactoring: the factor of
 * [[K11, K12], [K21, K22]] is the old factor with k rows under it, O(k N^2) against the N^3 / 3 of gp_set_data + gp_fit.
 * Xnew [k, D]; Yall [N + k, P] replaces ALL targets (the BO loop re-normalises them).  Hyper-parameters, Gower setting and
 * the jitter of the fit stay as they are; 1 <= k <= 128.  Always true fp64 ("emulate_fp64" does not apply).
 * 0: done -- *lml / *logdet (either may be NULL) of the grown model, gp_get_fit_state agrees.  L, the inverted diagonal tiles
 * and, where it was valid, the explicit inverse factor of the one-location path are extended and stay valid (an inverse factor
 * that did not exist is not built; the build rule of the *_rows entries goes on counting); the resident candidates stay,
 * everything else derived from the old factor or the old data -- Ky^-1, the candidates' posterior, the cached fmin, the sparse
 * fit, the ensemble -- is dropped and rebuilt by the call that needs it.
 * >0: the border's pivot was not positive or not finite (1-based row in the grown matrix); the context is left exactly as
 * before the call (N rows, fit valid), and the caller refits (gp_set_data + gp_fit, with its jitter ladder).
 * GP_ERR_STATE: no valid fit, or an output warp is on.  GP_ERR_ARG: k outside 1..128, a NULL argument.  Refusals leave the
 * context untouched. */
int gp_append(gp_t *gp, const double *Xnew, int64_t k, const double *Yall, double *lml, double *logdet);
/* borders written inside the last 128-row tile / into a new tile (a call that crosses a tile boundary counts once in each),
 * and calls refused or returned with a positive code, since gp_create */
int gp_append_stats(gp_t *gp, int64_t *in_place, int64_t *relayout, int64_t *refused);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) ---------------------
 * The candidate table shards across ranks; every rank holds a replica of the
 * fitted model.  uid is ncclUniqueId (128 bytes) produced on rank 0 and carried
 * to the other ranks by the launcher (any side channel). */
int gp_comm_unique_id(char *uid128);
int gp_comm_init(gp_t *gp, const char *uid128, int rank, int nranks);
int gp_comm_destroy(gp_t *gp);
/* rank / size as the RCCL communicator reports them (ncclCommUserRank, ncclCommCount) */
int gp_comm_info(gp_t *gp, int *rank, int *nranks);
/* all-gather of one (val, idx) pair per rank: vals[nranks], idxs[nranks]. */
int gp_comm_allgather_best(gp_t *gp, double val, int64_t idx, double *vals, int64_t *idxs);
/* ncclGetVersion of the librccl the process resolved (e.g. 22606): recorded by bench.py beside the mapped library path */
int gp_comm_version(int *version);
/* the top-k variant ("gather 8 x k pairs"): every rank contributes its k best (val, global idx) pairs
 * (idx < 0 marks an empty slot); all_vals / all_idxs [nranks * k], rank-major. */
int gp_comm_allgather_topk(gp_t *gp, int k, const double *vals, const int64_t *idxs, double *all_vals,
                           int64_t *all_idxs);
/* broadcast of a fitted model from root to all ranks: L, alpha, z, inverse tiles and the host-side scalars of the fit
 * (jitter, LML, log det), so that gp_fmin and gp_get_fit_state agree on every rank. */
int gp_comm_bcast_fit(gp_t *gp, int root);
/* Host-only self-test of gp_comm_bcast_fit's receiver side (no device, no communicator): packs the root's record from
 * root_state = {jitter, lml, logdet}, applies it to a scratch context standing in for a receiving rank with stale
 * results, and reports the receiver's {jitter, lml, logdet} and {fitted, fmin_valid, wi_valid, invp_valid, lr_valid,
 * predicted}.  Exists because RCCL with 2 ranks cannot run on a 1-GPU box (tests/test_host_logic.py). */
int gp_comm_selftest_fit_record(const double *root_state, double *state_out, int *flags_out);

/* ---- single-process multi-GPU: a device group ----------------------------------------------------------------------
 * The reference's BO loop is ONE Python process (GPyOpt/GPyOpt/core/bo.py:73-168, run.py:1207-1258) that scores a candidate
 * table and takes argmax / argsort()[:5] (run.py:1240-1241, GPyOpt/GPyOpt/optimization/anchor_points_generator.py:59-61).
 * A group lets that one caller thread use several GPUs of the node: one gp_t per entry of devices[] (the model replicated:
 * the fit does not shard, every member factors its replica, the devices side by side), the table cut into contiguous row
 * blocks -- member i of n takes rows [i M/n .., first M % n members one row longer] -- and the per-block winners merged with
 * NumPy's lowest-index tie rule.  With all devices different the members hold the communicators of ncclCommInitAll and
 * the winners travel by ONE grouped RCCL all-gather over xGMI, enqueued for every member by the calling thread inside
 * ncclGroupStart / ncclGroupEnd after every member has been validated (no member can wait on a peer that never joined; a
 * failed enqueue aborts the communicators and the group merges on the host from then on); with a device listed more than
 * once (a one-GPU box rehearsing the logic) the pairs are merged on the host, which gp_group_info reports.
 * STATUS: the RCCL route has not run on more than one device in any record of this repository -- no multi-GPU box was
 * available to the builder; what the tests execute is the host-merge route (devices = {0, 0, ...}) and the
 * single-member communicator.  Calls are synchronous; one group per caller thread. */
typedef struct gp_group gp_group_t;
int gp_group_create(gp_group_t **out, int ndev, const int *devices);
int gp_group_destroy(gp_group_t *grp);
/* ndev, whether the winners travel by RCCL, and a short note (<= cap bytes) saying which exchange is in use and why */
int gp_group_info(gp_group_t *grp, int *ndev, int *uses_rccl, char *note, int cap);
/* member i's context (owned by the group), e.g. for gp_get_alpha / gp_last_phases on one replica */
int gp_group_member(gp_group_t *grp, int i, gp_t **member);
/* gp_set_data / gp_set_params / gp_set_gower / gp_set_option applied to every member */
int gp_group_set_data(gp_group_t *grp, const double *X, const double *Y, int64_t N, int D, int P);
int gp_group_set_params(gp_group_t *grp, int kernel, int ard, double variance, const double *lengthscale, double noise);
int gp_group_set_gower(gp_group_t *grp, int enable, const int *is_discrete, const double *range);
int gp_group_set_option(gp_group_t *grp, const char *name, int64_t value);
/* gp_fit on every member at once; the scalars are member 0's, and a replica whose LML or jitter differs from member 0's in
 * any bit fails the call (GP_ERR_STATE) */
int gp_group_fit(gp_group_t *grp, int maxtries, double *lml, double *logdet, double *jitter_used);
int gp_group_fmin(gp_group_t *grp, double *fmin);
/* the WHOLE candidate table Xs[M, D]; each member keeps its block resident */
int gp_group_set_candidates(gp_group_t *grp, const double *Xs, int64_t M);
/* gp_acq_argbest / gp_acq_topk over the whole table: idx are rows of the table passed to gp_group_set_candidates */
int gp_group_acq_argbest(gp_group_t *grp, int type, double par, double fmin, double y_mean, double y_std, int sense,
                         int64_t *idx, double *val);
/* gp_acq_lp_argbest over the whole table (the local-penalisation batch loop of run.py:1238-1257): exclude[] holds rows of the
 * table passed to gp_group_set_candidates */
int gp_group_acq_lp_argbest(gp_group_t *grp, int type, double par, double fmin, double y_mean, double y_std, int transform,
                            const double *Xb, int nb, const double *r_x0, const double *s_x0, int sense,
                            const int64_t *exclude, int nex, int64_t *idx, double *val);
int gp_group_acq_topk(gp_group_t *grp, int type, double par, double fmin, double y_mean, double y_std, int sense, int k,
                      int64_t *idx, double *val);

/* The merge every layout applies to gathered (value, global row) pairs, as host-only helpers (no device needed): the best pair /
 * the k best in order, equal values lowest row first (np.argmax / np.argmin / a stable argsort on the unsharded vector); pairs with
 * idx < 0 are empty slots; a top-k tail that cannot be filled is idx = -1. */
int gp_merge_best(int n, const double *vals, const int64_t *idxs, int sense, int64_t *idx, double *val);
int gp_merge_topk(int n, const double *vals, const int64_t *idxs, int sense, int k, int64_t *idx, double *val);

/* ---- sparse GP (variational DTC) -------------------------------------------
 * GPy.models.SparseGPRegression (GPy/GPy/models/sparse_gp_regression.py:33-66) behind GPyOpt's GPModel(sparse=True)
 * (GPyOpt/GPyOpt/models/gpmodel.py:66-71): VarDTC inference over Mz inducing inputs Z, O(N Mz^2) instead of O(N^3).
 * Homoscedastic Gaussian noise, certain inputs, no mean function.  The sparse model lives on the same gp_t: it uses the
 * context's X, Y, kernel and parameters (gp_set_data, gp_set_params) and keeps buffers and a validity flag of its own.  No
 * sparse call reads or writes the exact model's state (factor, inverse factor, alpha, the resident candidates and their
 * results, the cached fmin): gp_fit / gp_predict after any sequence of sparse calls return the bits a fresh context returns.
 * Always true fp64 ("emulate_fp64" does not apply).  GP_ERR_STATE: no data or no parameters, the Gower option on, an output
 * warp on, fit before gp_sparse_set_inducing, the other calls before a sparse fit.  The acquisitions have sparse twins below
 * (gp_sparse_acq*, gp_sparse_*_rows: a candidate table, a cached posterior and a one-location path of the sparse model's own);
 * restarts in lockstep have a sparse entry of their own (gp_sparse_fit_grad_batch below); the exact model's batched restarts,
 * the sharded and group entries, the full covariance and posterior sampling stay exact-GP only. */
#define GP_SPARSE_MAX_INDUCING 2048
/* The inducing inputs Z [Mz, D], row-major (SparseGP.__init__ / set_Z, GPy/GPy/core/sparse_gp.py:53,69-74).  Drops the sparse
 * fit.  Z survives gp_set_params and a gp_set_data of the same D (which drop the sparse fit only); a gp_set_data with another
 * D drops Z as well.  GP_ERR_ARG: Mz outside 1..GP_SPARSE_MAX_INDUCING. */
int gp_sparse_set_inducing(gp_t *gp, const double *Z, int64_t Mz);
/* VarDTC.inference (var_dtc.py:66-216) with _compute_log_marginal_likelihood (:266-277): beta = 1 / max(noise, 1e-8), Kmm =
 * K(Z) + 1e-8 I, Lm = jitchol(Kmm), B = I + beta Lm^-1 Kuf Kfu Lm^-T, LB = jitchol(B) (linalg.py:56-81; the jitter each ladder
 * ended with in *jitter_kmm / *jitter_b, 0 when the first attempt succeeded; a failed ladder reports as gp_fit does).  Out
 * pointers may be NULL. */
int gp_sparse_fit(gp_t *gp, int maxtries, double *lml, double *jitter_kmm, double *jitter_b);
/* gp_sparse_fit and the gradients of its LML, one call per L-BFGS evaluation (SparseGP.parameters_changed and
 * _update_gradients, sparse_gp.py:76-119, over _compute_dL_dpsi / _compute_dL_dR, var_dtc.py:218-264):
 * dvariance, dlengthscale [1, or D with ard] = update_gradients_diag + update_gradients_full(dL_dKnm, X, Z) +
 * update_gradients_full(dL_dKmm, Z); dnoise = dL_dR, the derivative with respect to the noise variance by the reference's
 * formula also where the 1e-8 clamp is active; dZ [Mz, D] = gradients_X(dL_dKmm, Z) + gradients_X(dL_dKnm^T, Z, X).
 * The same inputs give the same bits on every call.  GP_ERR_ARG: P > 16. */
int gp_sparse_fit_grad(gp_t *gp, int maxtries, double *lml, double *dvariance, double *dlengthscale, double *dnoise, double *dZ);
/* gp_sparse_fit_grad for R members in ONE call: what the restarts of GPModel(sparse=True) in lockstep ask for
 * (GPyOpt/GPyOpt/models/gpmodel.py:78-93 over sparse_gp.py:76-119), one call per round of L-BFGS steps.
 * What a member computes: member r is gp_sparse_set_inducing(Z[r]) + gp_set_params(variance[r], lengthscale[r], noise[r]) +
 * gp_sparse_fit_grad over the context's X, Y, kernel family and ard (nls = 1, or D with ard, from the last gp_set_params): VarDTC
 * with both jitter ladders per member and beta = 1 / max(noise, 1e-8).  Z is [R, Mz, D], lengthscale [R, nls], dZ [R, Mz, D],
 * dlengthscale [R, nls], everything else [R].
 * Bits: member r's lml, jitter_kmm, jitter_b (those of gp_sparse_fit), dvariance, dlengthscale, dnoise and dZ are bitwise those
 * of the single call, whatever R is, whatever slot the member is in and whatever the other members are: a launch over members
 * runs the body of the single call's kernel (the same summation orders, fixed by constants and never by the grid, no float
 * atomics), with the member as blockIdx.z / .y or the GEMM's batch index, and the GEMM takes the instance it picks for one
 * member's tiles.  No launch of the sequence gives up the single call's bits at any accepted shape.  (woodbury_inv, which none of
 * these outputs depends on, is not formed.)
 * Status and failures: status[r] is 0, or the code gp_sparse_fit_grad returns for that member (a ladder that ended without a
 * factor); its outputs are then NaN.  A failed member does not fail the call.
 * Jitter ladders: in each ladder (Kmm, then B) only the members whose factorisation failed are factored again, alone with the
 * other failed members; runs of consecutive members share launches.  One copy of the members' info words and one
 * synchronisation per ladder round; the mean diagonal of B is fetched for failed members only.
 * GP_ERR_ARG: R outside 1..64; Mz outside 1..GP_SPARSE_MAX_INDUCING; a null pointer; a non-positive variance, lengthscale or
 * noise; P > 16; D and P beyond a workgroup's LDS in the gradient pass (as gp_sparse_fit_grad); more than
 * GP_SPARSE_BATCH_MAX_BYTES of buffers (below).  GP_ERR_STATE: no data or no parameters, the Gower option on, an output warp on.
 * Untouched state: the batch has buffers of its own, allocated at first use and owned by the context beside its other buffers.
 * It reads or writes none of: the resident inducing inputs, the resident sparse fit (woodbury vector and inverse, lml, gradient
 * weights), the sparse candidate table and its cached posterior, the cached sparse fmin, the exact model's factor, alpha, Ky^-1,
 * candidates and results, the exact batch's buffers, or any validity flag.  It needs no prior gp_sparse_set_inducing.
 * Always true fp64 ("emulate_fp64" does not apply).
 * Memory: per member 2 (n + 128) n + 10 n^2 + 3 Npad n doubles and the small vectors, n = Mz rounded up to 128 -- 0.5 GB at
 * N = 16384, Mz = 1024.  GP_SPARSE_BATCH_MAX_BYTES is a policy cap, not a measurement: 16 GiB is a sixteenth of the device's
 * 288 GB, leaves the exact model, its candidates and several contexts their room beside it, and still takes 30 such members --
 * six rounds' worth of GPyOpt's five restarts.  gp_sparse_batch_bytes reports what a call would allocate (the same checks of R
 * and Mz, nothing allocated), so that a caller decides without restating the formula. */
#define GP_SPARSE_BATCH_MAX_BYTES (16LL << 30)
int gp_sparse_fit_grad_batch(gp_t *gp, int R, int64_t Mz, const double *Z, const double *variance, const double *lengthscale,
                             const double *noise, int maxtries, double *lml, double *jitter_kmm, double *jitter_b,
                             double *dvariance, double *dlengthscale, double *dnoise, double *dZ, int *status);
int gp_sparse_batch_bytes(gp_t *gp, int R, int64_t Mz, int64_t *bytes);
/* Posterior.woodbury_vector [Mz, P] (Cpsi1Vf, var_dtc.py:142,199) and woodbury_inv [Mz, Mz] = Lm^-T (I - B^-1) Lm^-1
 * (var_dtc.py:209-212) of the sparse fit; either may be NULL. */
int gp_sparse_posterior(gp_t *gp, double *woodbury_vector, double *woodbury_inv);
/* Posterior._raw_predict (posterior.py:225-248) at Xs [M, D], given by value: mean [M, P] = Kx w, var [M] = k** - diag(Kx
 * woodbury_inv Kx^T) clipped below at 1e-15, then + noise with include_noise (gaussian.py:102-110).  dmdx [M, D, P] and dvdx
 * [M, D] (either may be NULL): GP.predictive_gradients over _predictive_variable = Z (gp.py:407-454); the gradients are not
 * clipped.  Candidates go in chunks of "mc_max" rows.  A row's results do not depend on the rows it is predicted with (table
 * size, position, chunk): the same row gives the same bits in any table, and the same table the same bits on every call.  The
 * exact model's resident candidate block (gp_set_candidates) is not touched. */
int gp_sparse_predict(gp_t *gp, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                      double *dvdx);
/* min over the training inputs of the sparse posterior mean Kfu w, first output column (GPModel.get_fmin, gpmodel.py:125-129) */
int gp_sparse_fmin(gp_t *gp, double *fmin);

/* -- acquisitions over the sparse posterior.  Argument conventions are those of the exact entries: out holds the NEGATED
 * acquisition, y_mean / y_std undo a Standardize normaliser, transform is 0 or 1, lp != 0 adds the local penalisation of
 * gp_acq_lp over the batch Xb [nb, D], r_x0, s_x0 (nb = 0: the un-penalised log acquisition).  All need P = 1.  GP_ERR_STATE: what
 * gp_sparse_predict refuses, and a table entry before gp_sparse_set_candidates; GP_ERR_ARG: P != 1, an unknown acquisition, a bad
 * sense / k / exclude / batch, M < 1.  None of them reads or writes the exact model's state (its candidates, posterior, scores). */

/* The sparse model's resident candidate table Xs [M, D], in a buffer of its own.  Its posterior is cached lazily by the scoring
 * entries below -- mean and variance (noise included, as GPModel.predict asks, gpmodel.py:102), gradients once asked for -- and
 * is, bit for bit, what gp_sparse_predict(include_noise = 1) returns for those rows.  Whatever drops the sparse fit drops the
 * cache; the table survives as Z does (another D drops it).  gp_sparse_predict, gp_sparse_fmin and the two rows entries leave table
 * and cache intact.  Needs data (GP_ERR_STATE). */
int gp_sparse_set_candidates(gp_t *gp, const double *Xs, int64_t M);
/* gp_acq / gp_acq_grad (lp = 0) or gp_acq_lp / gp_acq_lp_grad (lp != 0) on the table: out [M] and, when given, dout [M, D].  A
 * row's score depends on its own posterior only: the same row gives the same bits in any table, at any position. */
int gp_sparse_acq(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int lp, int transform,
                  const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out, double *dout);
/* gp_acq_argbest / gp_acq_lp_argbest of the same vector: sense, ties (lowest index), exclude as there. */
int gp_sparse_acq_argbest(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int lp, int transform,
                          const double *Xb, int nb, const double *r_x0, const double *s_x0, int sense, const int64_t *exclude,
                          int nex, int64_t *idx, double *val);
/* gp_acq_topk: 1 <= k <= GP_TOPK_MAX, equal scores lowest index first, idx = -1 in the tail when M < k. */
int gp_sparse_acq_topk(gp_t *gp, int type, double par, double fmin, double y_mean, double y_std, int sense, int k, int64_t *idx,
                       double *val);

/* A handful of locations per call, given by value: the acquisition optimiser's inner loop over a sparse model (see gp_predict_rows
 * / gp_acq_rows for the exact model's twins and the argument rules: mean / var may be NULL, dvdx needs dmdx, dmdx alone comes
 * without mean / var and is estimate_L's inner call, which needs the woodbury vector only).  For M <= option "small_m" (8)
 * locations the call is ONE launch per pass with no copy commands (csrc/sparse_rows.hip): k = K(x, Z) generated into LDS, b =
 * woodbury_inv k from one read of the Mz x Mz matrix for all locations of the pass, var = max(kss - k . b, 1e-15) (+ noise), the
 * two gradients_X sums, the acquisition and the penaliser, written into a pinned result block.  A pass takes the locations that
 * fit the kernel arguments (M D <= 128: all eight up to D = 16, two at D = 64).  A location's results are the same bits whatever
 * its slot, its company and M (1 .. 8), and on every call.  More locations go through the table arithmetic on scratch buffers --
 * the bits of gp_sparse_predict -- never through the resident table.  Fused path and table path agree to rounding, not bitwise:
 * they contract in a different order (tests/test_gpu_sparse_acq.py).  gp_sparse_predict itself keeps the table arithmetic for
 * every M, as its own contract asks. */
int gp_sparse_predict_rows(gp_t *gp, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                           double *dvdx);
int gp_sparse_acq_rows(gp_t *gp, const double *Xs, int64_t M, int type, double par, double fmin, double y_mean, double y_std,
                       int lp, int transform, const double *Xb, int nb, const double *r_x0, const double *s_x0, double *out,
                       double *dout);
/* how many of those calls took the fused path / the table arithmetic since gp_create (route checks of the tests) */
int gp_sparse_rows_stats(gp_t *gp, int64_t *fused, int64_t *fallback);

/* -- the joint posterior of the sparse model (csrc/api_sparse_cov.hip).  All four entries refuse what gp_sparse_predict refuses
 * (GP_ERR_STATE: no sparse fit, a mean function resident, a dead context), a null pointer and a count below 1 (GP_ERR_ARG); a
 * refused call leaves the context as it was.  They work on buffers of the sparse model's own: the exact model's candidates,
 * posterior and results, the sparse candidate table with its cached posterior and the cost snapshot are neither read nor written. */

/* full_cov = True of Posterior._raw_predict over _predictive_variable = Z (posterior.py:229-232) at Xs [M, D], given by value:
 * mean [M, P] (may be NULL) and cov [M, M] = K(Xs, Xs) - K(Xs, Z) woodbury_inv K(Z, Xs), + noise I with include_noise
 * (gaussian.py:104-105).  Formed as K(Xs, Xs) - U U^T + T T^T with U = K(Xs, Z) Lm^-T and T = U LB^-T (woodbury_inv = Lm^-T
 * (I - B^-1) Lm^-1): lower tiles, mirrored -- cov is bitwise symmetric, and the same call gives the same bits.  Unlike
 * gp_sparse_predict's variance the diagonal is not clipped.  GP_ERR_ARG: M rounded up to the tile (128) beyond "mc_max". */
int gp_sparse_predict_full_cov(gp_t *gp, const double *Xs, int64_t M, int include_noise, double *mean, double *cov);
/* gp_posterior_samples over that covariance: dev [S, M], dev[s, :] = C z_s with C C^T = cov (+ jitter I) factored on the device
 * under jitchol's ladder (mean of cov's diagonal x 1e-6 x 10^k, at most maxtries steps; *jitter_used is 0 when none was needed)
 * and z_s = Z[s, :] the caller's standard normals, Z [S, M].  mean [M, P] (may be NULL) is bitwise the mean of
 * gp_sparse_predict_full_cov.  GP_ERR_NOT_PD_DIAG: the first attempt failed and cov has a non-positive diagonal entry; a positive
 * code: the ladder ended without a factor.  GP_ERR_ARG also for M beyond "mc_max" as above. */
int gp_sparse_posterior_samples(gp_t *gp, const double *Xs, int64_t M, int include_noise, const double *Z, int S, int maxtries,
                                double *mean, double *dev, double *jitter_used);
/* A second point set X2 [R, D], 1 <= R <= "mc_max", made resident for gp_sparse_cov_between.  G = K(X2, Z) woodbury_inv is built
 * by the first gp_sparse_cov_between after a fit or a new point set and kept: whatever drops the sparse fit drops G, the points
 * stay as the candidate table does (another D drops them).  Needs data (GP_ERR_STATE), not a fit. */
int gp_sparse_cov_set_points(gp_t *gp, const double *X2, int64_t R);
/* cov [M1, R], cov[i, r] = k(x1_i, x2_r) - sum_j G[r, j] k(x1_i, z_j): the posterior covariance (no noise) between the locations
 * X1 [M1, D], given by value, and the resident points.  Up to 8 locations are ONE launch per pass with no copy commands (the
 * locations in the kernel arguments, M1 D <= 128 per pass, the result in a pinned block); more go through the same kernel body
 * in blocks of eight.  Every entry has one writer and a fixed summation order: a location's row has the same bits whatever M1,
 * its position and its company, its first R' entries the same bits as against the first R' points alone, and the same call the
 * same bits.  GP_ERR_STATE also before gp_sparse_cov_set_points. */
int gp_sparse_cov_between(gp_t *gp, const double *X1, int64_t M1, double *cov);

/* ---- ensemble: S hyper-parameter members with resident posteriors, acquisitions integrated over them ----------------
 * GPModel_MCMC (GPyOpt/GPyOpt/models/gpmodel.py:180-355) with acquisitions/{EI,MPI,LCB}_mcmc.py.  An ensemble is S members
 * over the context's (X, Y), each with hyper-parameters of its own (an HMC sample, gpmodel.py:243-262); it is kept beside the
 * context's own fit and independent of it.  gp_set_data drops it; gp_set_params, gp_fit and gp_set_candidates do not, and no
 * ensemble entry touches the context's fit, candidate posterior or parameters.  Always true fp64.  Kernels: csrc/ens_rows.hip.
 *
 * GP_ERR_ARG: S outside 1..64, Npad > 2048 (the batched fit's caps), P != 1, M outside 1..8 of the rows entries, an unknown
 * acquisition, a bad sense.  GP_ERR_STATE: no data or parameters, the Gower option on (the lengthscale does not enter a Gower
 * K), an output warp on, a scoring call before a valid gp_ens_fit, a table call before gp_set_candidates. */

/* Replaces the model.param_array = sample; model._trigger_params_changed() of every call (gpmodel.py:266-272, 285-291, 307-315):
 * the S members are factored ONCE, in lockstep, with the launch sequences and the per-member jitter ladder of
 * gp_fit_grad_batch, and each member's alpha, explicit inverse factor, parameters, jitter and fmin are KEPT.  lengthscale is
 * [S, nls] with nls of the last gp_set_params (kernel family and ard come from there too).  fmin[z] = min over the training
 * inputs of member z's posterior mean (get_fmin, gpmodel.py:285-291).  lml / logdet / jitter_used / fmin may be NULL.  A
 * member that cannot be factored after maxtries fails the whole call with gp_fit's not-positive-definite code; the ensemble
 * is then invalid. */
int gp_ens_fit(gp_t *gp, int S, const double *variance, const double *lengthscale, const double *noise, int maxtries, double *lml,
               double *logdet, double *jitter_used, double *fmin);
/* *S = members of the valid ensemble, 0 when there is none. */
int gp_ens_info(gp_t *gp, int *S);
/* GPModel_MCMC.predict / predict_withGradients (gpmodel.py:264-276, 293-323) without the clip: every member's posterior at
 * M <= 8 locations given by value, mean / var [S][M] (either may be NULL), dmdx / dvdx [S][M][D] (both or neither).  Member z's
 * numbers are, bit for bit, gp_predict_rows' on a context fitted with z's parameters: whatever S, z's position and the other
 * locations of the call.  The launches of a call do not depend on S (the member is a grid dimension). */
int gp_ens_predict_rows(gp_t *gp, const double *Xs, int64_t M, int include_noise, double *mean, double *var, double *dmdx,
                        double *dvdx);
/* AcquisitionEI_MCMC / MPI_MCMC / LCB_MCMC ._compute_acq[_withGradients] (EI_mcmc.py:32-59, MPI_mcmc.py:32-59,
 * LCB_mcmc.py:33-60), negated as gp_acq_rows returns it: the mean over members of the rule (csrc/acq_math.h) at the member's own
 * fmin, mean and std = sqrt(max(var + noise, 1e-10)), dstd = dvar / (2 std) (gpmodel.py:313-317); no normaliser.  out [M],
 * dout [M, D] or NULL, M <= 8.  Members are added in member order: bitwise repeatable. */
int gp_ens_acq_rows(gp_t *gp, const double *Xs, int64_t M, int type, double par, double *out, double *dout);
/* The same value over the table made resident by gp_set_candidates, any M: one cross covariance per member, one batched GEMM
 * against the inverse factors, one reduce.  Agrees with gp_ens_acq_rows to rounding (another contraction order). */
int gp_ens_acq(gp_t *gp, int type, double par, double *out);
/* arg-best of that vector: sense +1 largest, -1 smallest; ties go to the lowest index. */
int gp_ens_acq_argbest(gp_t *gp, int type, double par, int sense, int64_t *idx, double *val);

/* ---- entropy search ------------------------------------------------------------------------------------------------------
 * AcquisitionEntropySearch (GPyOpt/GPyOpt/acquisitions/ES.py) with util/epmgp.py: a belief over which of R representer points is
 * the minimum, and for every candidate the expected change of that belief's entropy.  The device takes the representers'
 * posterior, the EP sweeps of p_min and the scoring of candidate tables; the closing algebra of min_faktor (epmgp.py:166-208)
 * and the renormalisation of joint_min (:92-119) stay on the host (R solves of order R - 1), which hands the belief back with
 * gp_es_set_belief.  Exact single-output model only.  Always true fp64 ("emulate_fp64" covers the candidate solve of the table
 * as for gp_predict, never the kernels of csrc/es.hip).
 * State: representers and belief belong to the fit they were made with; everything that drops or changes the fit (gp_set_data,
 * gp_set_params, gp_set_gower, gp_kernel_matrix, every gp_fit*, gp_append, gp_set_output_warp, gp_comm_bcast_fit) drops both, and
 * scoring without them is GP_ERR_STATE -- never a score from a stale belief.  GP_ERR_STATE as well: no fit, an output warp on, a
 * sparse fit or an ensemble held by the context.  GP_ERR_ARG: R outside 1..GP_ES_MAX_R, S outside 1..GP_ES_MAX_S, P > 1. */
#define GP_ES_MAX_R 64
#define GP_ES_MAX_S 1024
/* ES._update_parameters' model calls (ES.py:105-108): Xr [R, D] becomes resident with V_R = L^-1 K(X, Xr) (a padded 128 x Npad
 * block); mu [R] and cov [R, R] receive the representers' posterior mean and full covariance WITH noise (posterior.py:280-284,
 * gaussian.py:104-105), un-normalised as mean y_std + y_mean, cov y_std^2.  No floor is applied (GPModel._predict applies its
 * 1e-10 on the host).  The resident candidates stay; their cached posterior is dropped.  Drops an earlier belief. */
int gp_es_set_representers(gp_t *gp, const double *Xr, int R, double y_mean, double y_std, double *mu, double *cov);
/* The EP sweeps of min_faktor / lt_factor / log_relative_gauss (epmgp.py:122-153, 211-288) for the R chains "representer k is the
 * minimum" of the Gaussian (mu [R], cov [R, R]) given by value: a pure function of its arguments that needs no data and no fit.
 * One workgroup per chain, its working mean and covariance in LDS, the factors visited in the reference's order, the
 * reference's thresholds (|z| > 6, float32 eps, + 1e-25 under the root), at most max_sweeps sweeps (the reference: 50), stopped
 * where a sweep's sum |d| < tol (the reference: 1e-3) or at the first NaN d.  Out, per chain k: the site parameters P, MP, logS
 * [R, R - 1]; status[k] = 0 converged, 1 sweep limit, -1 a factor ended the chain (exit_flag -1 or a NaN d: the reference yields
 * logZ = -inf and zero derivatives), -2 NaN in V (the reference raises); sweeps[k] = sweeps begun. */
int gp_es_pmin(gp_t *gp, const double *mu, const double *cov, int R, int max_sweeps, double tol, double *P, double *MP,
               double *logS, int *status, int *sweeps);
/* The belief over the resident representers: logP [R], the representers' log-proposal values u [R], G [R, R] = dlogPdMu,
 * Q [R, R, R] with Q_i = (H_i + H_i^T) / 4 - (T_i + T_i^T) / 2 (H = dlogPdMudMu, T_i = dlogPdSigma[i] unpacked into the lower
 * triangle in row-major order, diagonal whole), so that m^T Q_i m is ES.py:148-154's deterministic change for the innovation m;
 * W [S] the normal quantiles of ES.py:76-78.  GP_ERR_STATE: no representers, or R differs from theirs. */
int gp_es_set_belief(gp_t *gp, const double *logP, const double *u, const double *G, const double *Q, int R, const double *W,
                     int S);
/* ES._compute_acq (ES.py:124-170) over the resident candidates, negated as acquisition_function returns it: out [M].  Per chunk
 * of the candidate solve C = K(Xs, Xr) - (K(Xs, X) L^-T) V_R^T; the candidate's variance without noise, floored at 1e-10 after
 * un-normalising (gpmodel.py:99 through ES.py:199); m = C / s, det_i = m^T Q_i m, g_i = G_i . m; for each w of W the log-sum-exp
 * over i of logP_i + det_i + g_i w (the maximum instead where any w of the candidate gives an infinite one, ES.py:162-163),
 * dHp = sum_i e^l (l + u_i); out = -mean_w dHp.  y_std as in gp_acq.  Fixed summation order, no atomics: a candidate's value
 * does not depend on M or on its row. */
int gp_es_acq(gp_t *gp, double y_std, double *out);
/* arg-best of that vector: sense +1 largest, -1 smallest; ties go to the lowest index. */
int gp_es_acq_argbest(gp_t *gp, double y_std, int sense, int64_t *idx, double *val);
/* gp_set_candidates + gp_es_acq for the locations Xs [M, D] given by value: what the acquisition optimiser asks for (ES has no
 * analytic gradient, so L-BFGS-B differences D + 1 one-location calls per step).  For M <= option "small_m" (8) locations that
 * fit the fused rows path (see gp_predict_rows: the same rules, the same build policy of the inverse factor) a pass is the path's
 * forward launch over L^-1 -- w = L^-1 k* -- and ONE more kernel: C = k(x, Xr) - V_R w, the variance kss - |w|^2, the score, into
 * the pinned result block behind the pass's ticket; no copy commands either side.  A location's value is the same bits whatever
 * its slot and its company.  Otherwise the call is the two table calls.  The routes agree to rounding (tests: 1e-9) and both
 * count in gp_rows_stats.  The resident candidate block is unspecified afterwards. */
int gp_es_acq_rows(gp_t *gp, const double *Xs, int64_t M, double y_std, double *out);

/* ---- measurement ---------------------------------------------------------
 * Phase timings of the last gp_fit / gp_predict measured with HIP events on the
 * library's stream; names[i] is a static string, ms[i] milliseconds, flops[i] the
 * algorithmic flop count of the phase (0 for bandwidth phases), bytes[i] its
 * algorithmic bytes.  Returns the number of phases written (<= cap). */
int gp_last_phases(gp_t *gp, int cap, const char **names, double *ms, double *flops, double *bytes);
/* Dominant-kernel accounting (the fp64 MFMA GEMM): launches, summed device time (ms, HIP events around the launches
 * when profiling is on), algorithmic flops.  With the default threshold the events bracket exactly the launches of one
 * kernel symbol, gemm_nt_kernel<1, 128, 4, false, 128> (C -= A B^T, >= 1400 output tiles), so that the average agrees with that
 * symbol's row of a rocprofv3 --stats summary; "profile_min_tiles" < 1024 brackets every launch above it instead
 * (tracing tools).  Reset by gp_profile(gp, 1).  gp_profile(gp, 2) brackets the launches of the second fp64 symbol instead,
 * gemm_nt_kernel<1, 64, 2, false, 64> (the same update as 64 x 64 work units: the factorisation chain's in-panel and
 * look-ahead updates, short candidate updates); events around those ~100-us launches stall the chain, so this is for a
 * pass outside any timed region. */
int gp_profile(gp_t *gp, int on);
int gp_gemm_stats(gp_t *gp, int64_t *launches, double *ms, double *flops);
/* the same for the residue GEMM of "emulate_fp64" (rns_gemm256_kernel, every launch): launches, summed device time, int8
 * operations (2 per multiply-add of the blocks a launch computes) */
int gp_rns_stats(gp_t *gp, int64_t *launches, double *ms, double *ops);
/* wall time (ms) during which at least one profiled launch was running: the union of their intervals.  Launches of
 * gp_fit_predict overlap, so the SUM of durations above counts shared time twice; flops / busy is the kernel's
 * throughput while it runs. */
int gp_gemm_busy(gp_t *gp, double *busy_ms);
/* per-launch record of the profiled GEMM launches: output tiles, K (negative: triangular contraction), ms */
int gp_gemm_trace(gp_t *gp, int cap, int64_t *tiles, int *K, double *ms);
int gp_synchronize(gp_t *gp);
/* Test hook: ONE launch of the fp64 GEMM (csrc/gemm.hip) on host operands, through the instance selection and the options every
 * launch of the context takes.  mode 0: C = A B^T, 1: C -= A B^T over the 128 x 128 output tiles (i, c), c in [c0, c1), i in
 * [tri ? c : r0, r1), contraction length K (a multiple of 16).  C and A are [r1 * 128, ld], B is [c1 * 128, ld], row-major with one
 * even pitch ld >= max(K, c1 * 128); r1, c1 <= 256.  Tiles outside the set keep their C. */
int gp_debug_gemm(gp_t *gp, int mode, double *C, const double *A, const double *B, int64_t ld, int K, int r0, int r1, int c0,
                  int c1, int tri);
/* Tunables (none changes a result beyond rounding; tests/test_gpu_random_shapes.py sweeps the blocking ones):
 *   "panel_tiles"        outer panel width of the factorisation and of the inverted panels, in 128-tiles (default 6)
 *   "lookahead"          0/1: one panel of look-ahead on separate streams (default 1)
 *   "lookahead_min_tiles"  gp_fit alone: matrices of at most this many 128-tiles (default 40, N <= 5120) take the same
 *                        factorisation on ONE stream (bitwise the same factor; the look-ahead's per-panel events cost more there)
 *   "mc_max"             candidate rows per chunk (default 16384)
 *   "small_below", "chain_small_below"   launches with fewer 128-tiles run as 64x64 work units (1400 / 400 on the chain)
 *   "waves8", "stagger", "trsm_rows64", "supertile"   GEMM launch shape
 *   "gemm_sched"         K loop of the 8-wave GEMM instance (launches of >= "long_min_tiles" output tiles): 1 = every fragment read,
 *                        staging load and LDS write at a fixed place between two MFMAs (gemm_nt_sched_kernel), 0 = the plain loop
 *                        (gemm_nt_kernel<., 128, 4, false, 128>).  Bitwise the same results; the paired triangular-K twin always
 *                        runs the plain loop, and so do the launches on the look-ahead factorisation's side streams unless
 *                        "gemm_sched_side" = 1 (default 0: beside the latency chain the step is slower with it).  "long_min_tiles" (default 1024, >= 1): the tile count from which a launch takes the
 *                        8-wave instance and the stagger; 1 with "small_below" = "chain_small_below" = 0 sends every launch there
 *   "pipe_stages", "pipe_start_pct"   gp_fit_predict: how many candidate stages ride behind the factorisation (0 = automatic:
 *                        14 % of the panels, 3 at N = 16384) and
 *                        after which share of its panels they are released (-1 = automatic: 32 up to 24 panels, 40 beyond)
 *   "pipe_stages_grad", "pipe_start_pct_grad"   the same for gp_fit_grad (0 = automatic: 36 % of the panels; 40)
 *   "lauum_panels"       Ky^-1 product accumulated per k-panel (default 1)
 *   "pair_tri"           triangular-K products: column tiles paired for equal contraction length (default 2)
 *   "fmin_direct"        gp_fmin through the N^2 product K(X,X) alpha instead of y - d alpha (default 0)
 *   "emulate_fp64"       0/1 (default 0; environment GPHIP_EMULATE_FP64 sets the default of new contexts): the candidate
 *                        solve's updates T[:, > J] -= S_J L[> J, J]^T (dtrtrs, posterior.py:294; 95 % of gp_predict's flops)
 *                        and, with "emulate_fit" (default 1), the factorisation's trailing update (dsyrk/dgemm inside dpotrf,
 *                        linalg.py:58) and Ky^-1 (dtrtri + dpotri, linalg.py:127-145) run on the int8 matrix cores in residue form (csrc/rns.hip): operands as 52-bit
 *                        fixed point, 14 moduli, exact int32 accumulation, CRT reconstruction once per column.  Same results
 *                        to ~1e-12 (only the operands are rounded, to one fp64 ulp of the largest entry); diagonal tiles,
 *                        panel solves and all reductions stay true fp64; gp_fit_predict then runs fit and predict one after
 *                        the other.  Non-finite data cannot be put into fixed point: the call then repeats the step in
 *                        true fp64 (NaNs propagate as in the reference).  "rns_group" / "rns_group_fit" (default 8, 1..16): panels per residue launch of the
 *                        candidate solve / of the trailing update; "rns_interleave" (default 1, process-wide): the eight
 *                        XCDs work on one modulus at a time.  Results do not depend on these three.
 *   "inner_tiles"        tile columns per step of the in-panel factorisation: 1 (default) = diagonal tile, panel solve, K = 128 update;
 *                        2 = a 256 x 256 diagonal block per launch (potrf_pair_kernel), both tile columns of the rows below per launch
 *                        (trsm2_kernel), one K = 256 update -- half the dependent launches, the same wall time;
 *                        "inner_min_rows": two columns only while at least this many row tiles lie below (default 0)
 *   "own_keep_per_row"   look-ahead factorisation: of a trailing update with n row tiles below the look-ahead panel the masked bulk stream keeps
 *   "own_keep_base"      own_keep_base + own_keep_per_row * n * panel_tiles / 6 tiles (what lasts as long as the chain is busy with that panel; defaults 200 and
 *                        36); the rest, the far tile columns, is updated on the chain stream -- every CU -- in the window in which the chain
 *                        would wait for the bulk stream.  Same bits as without; own_keep_per_row = 0 switches it off.
 *                        "own_keep_pipe_pct" (default 0): the kept share in per cent of the rule's once the pipelined candidate stages of
 *                        gp_fit_predict / gp_fit_grad share the bulk stream's CUs
 *   "small_m"            up to this many candidates (default 8, 0 = never) are solved as matrix-vector work bound by one read of L
 *                        (csrc/smallm.hip: the acquisition optimiser's one-row calls) instead of through the 128-row tile path;
 *                        gp_predict_full_cov / gp_posterior_samples always take the tile path
 *   "rows_wide"          1 (default): a gp_*_rows call of 5 .. 8 locations with M D <= 128 is ONE pass over the inverse factor
 *                        (csrc/onerow.hip, the wide instances); 0: passes of four locations.  The same bits either way
 *   "debug_potrf_lds"    test hook, process-wide: extra dynamic LDS requested with every diagonal-tile launch (a refused launch beyond
 *                        ~9 KB: what the launch checks are tested with)
 *   "profile_min_tiles"  see gp_profile
 * The number of CUs kept free of the trailing update for the look-ahead chain is fixed per process
 * (environment GPHIP_RESERVE_CUS, default 32; "reserve_cus" only checks the value). */
int gp_set_option(gp_t *gp, const char *name, int64_t value);

/* ---- cost-aware EI / MPI: the evaluation-time cost model (GPyOpt/core/task/cost.py, acquisitions/base.py:33-50) ------------
 * The cost is exp(m_c(x)), m_c the posterior mean of a second GP over the logarithm of the evaluation times.  A posterior mean
 * needs no factor:  m_c(x) = shift + scale sum_j alpha_j k(x, Xc_j),  so the cost surface is the snapshot (Xc, alpha, kernel
 * parameters, normaliser) and any handle can own a copy.
 *
 * gp_cost_set copies the surface into buffers of the context's own (no pointer to another handle is kept): Xc [Nc, D] with D
 * the handle's, alpha [Nc] (gp_get_alpha of the cost GP), kernel one of GP_KERNEL_* (Euclidean, ARD or not: lengthscale [D] or
 * [1]), shift / scale the cost GP's output normaliser (its y_mean / y_std; 0 and 1 without one).  Nc = 0 clears the surface.  It
 * needs gp_set_data (GP_ERR_STATE: D is the data's), is valid before or after gp_fit, and touches neither the fit nor the
 * posterior caches; gp_set_data with another D drops the surface.  GP_ERR_ARG: a null pointer, Nc < 0, an unknown kernel, a
 * variance or lengthscale that is not positive and finite, a non-finite shift or scale.
 * gp_cost_info: *Nc = rows of the resident surface, 0 when there is none.
 * gp_cost_rows: logc [M] = m_c at the M locations Xs [M, D] and, when dlogc is given, its x-gradient [M, D].  GP_ERR_STATE
 * without a surface.  The terms of a location are summed in ONE order (chunks of 32 rows in row order, the chunks in order): its
 * bits do not depend on M, on its row, or on whether it came in a table (M > 8, or the resident candidates of a flagged scoring
 * call) or among a few rows.  The Exponential family keeps the _inv_dist convention: a location that coincides with an Xc_j
 * takes 0 from it into the gradient.
 *
 * GP_ACQ_PER_COST in the `type` of gp_acq, gp_acq_grad, gp_acq_argbest, gp_acq_topk, gp_acq_rows, gp_sparse_acq,
 * gp_sparse_acq_argbest, gp_sparse_acq_topk, gp_sparse_acq_rows, gp_ens_acq, gp_ens_acq_argbest and gp_ens_acq_rows divides the
 * negated scores by c = exp(logc): neg <- neg / c, dneg <- (dneg - neg dlogc) / c (for the ensemble after the average over the
 * members).  GP_ERR_ARG: no surface, LCB (LCB.py takes no cost), a penalised call (lp: LP.py:27 builds the penalised acquisition
 * with unit cost).  The entropy-search entries, the penalised-only entries (gp_acq_lp*) and the group entries take no flag.  The
 * logc of a resident table is computed once per table and surface: values, arg-best and top-k of one table pay the pass once. */
int gp_cost_set(gp_t *gp, const double *Xc, int64_t Nc, const double *alpha, int kernel, int ard, double variance,
                const double *lengthscale, double shift, double scale);
int gp_cost_info(gp_t *gp, int64_t *Nc);
int gp_cost_rows(gp_t *gp, const double *Xs, int64_t M, double *logc, double *dlogc);

/* ---- mean function: an affine trend m(x) = x^T A + b under the exact GP ------------------------------------------------------
 * GPRegression(..., mean_function=...) over GPy's mappings.Linear, mappings.Constant and their Additive sum (core/gp.py:89-95,
 * 267-271, 293-294; exact_gaussian_inference.py:42-50, 74): the fit runs on Y - m(X), m(x*) is added to the posterior mean, and
 * dL/dm = alpha is pushed through the mapping's update_gradients.
 *
 * gp_mean_set copies A [D, P] (row-major) and b [P] into a buffer of the context's own; either may be NULL (a part that is not
 * there), both NULL clears the mean.  It needs gp_set_data (GP_ERR_STATE: D and P are the data's), is refused while an output warp
 * is on (GP_ERR_STATE) and for a non-finite entry (GP_ERR_ARG), and drops what gp_set_params drops: the fit, the cached posterior
 * and fmin, representers and belief.  The mean survives gp_set_params and a gp_set_data with the same D and P; another D or P drops
 * it.  While a mean is resident the context keeps the raw targets beside the residuals Y - X A - 1 b^T, which are rebuilt before the
 * next factorisation whenever the data or the mean changed -- per element from b_p, the D products in dimension order by fma, so
 * the same inputs give the same bits on every call -- and gp_fit, gp_fit_grad, gp_lml_grad and gp_fit_predict run unchanged on
 * them: LML, log det, alpha and the hyper-parameter gradients are GPy's with YYT_factor = Y - m.  Always true fp64
 * ("emulate_fp64" does not apply).  (gp_get_targets hands out what the fit reads: once a fit has run, these residuals.)
 * gp_mean_info: *has_A / *has_b = 1 where that part is resident (either pointer may be NULL).
 * gp_mean_grad: dA [D, P] = X^T alpha, db [P] = 1^T alpha of the current fit (either may be NULL; GP_ERR_STATE before a fit; valid
 * with or without a resident mean).  A two-level sum over N whose order is fixed by one constant (chunks of 256 rows in row order,
 * the chunks in order): bitwise repeatable, no atomics.
 *
 * Posterior: m(x*) joins the mean where it is formed -- behind the reduction of every table route (gp_predict, gp_fit_predict,
 * gp_predict_full_cov, gp_posterior_samples and the cache the scoring entries read), inside the finish pass of the fused rows
 * route (gp_predict_rows, gp_acq_rows: instances of their own) -- and A joins dmdx (gp_predict_grad, the rows entries).  So EI /
 * LCB / MPI values and gradients, arg-best, top-k, the penalised entries and GP_ACQ_PER_COST see the full mean, and gp_fmin is
 * min_i (y_i - (noise + 1e-8 + jitter) alpha_i) over the RAW targets.  A Gower model takes a mean as any other: m never enters K.
 * With no mean resident every kernel is launched as before and returns the same bits.
 *
 * Refused while a mean is resident (GP_ERR_STATE, the message names the mean function, nothing is launched, the context stays
 * usable): gp_set_output_warp, gp_warp_grad, gp_fit_grad_warp, gp_predict_warped; the gp_sparse_*, gp_ens_* and gp_es_* entries
 * (their counters gp_sparse_rows_stats and gp_ens_info still answer); gp_append; gp_fit_grad_batch, gp_fit_grad_x_batch,
 * gp_fit_grad_warp_batch; gp_lml_grad_x, gp_fit_grad_x, gp_set_candidates_kumar; the gp_group_* entries that touch data, fit or
 * scores, and gp_comm_init, gp_comm_allgather_best, gp_comm_allgather_topk, gp_comm_bcast_fit.  Their prediction sides do not add
 * m, or they read the fit's targets as the data. */
int gp_mean_set(gp_t *gp, const double *A, const double *b);
int gp_mean_info(gp_t *gp, int *has_A, int *has_b);
int gp_mean_grad(gp_t *gp, double *dA, double *db);

/* ---- black-box constraints: feasibility-weighted EI / MPI (Gardner et al. 2014; Gelbart et al. 2014) ---------------------------
 * K <= GP_FEAS_MAX constraints c_k(x) <= bound[k] are known through evaluations only; each is modelled by a GP of its own, and
 * the acquisition is weighted by the probability of feasibility
 *     F(x) = prod_k Phi(z_k),   z_k = (bound[k] - m_k(x)) / s_k(x),
 * m_k = mean c_std[k] + c_mean[k] and s_k = sqrt(max(var c_std[k]^2, 1e-10)) the un-normalised predictive mean and standard
 * deviation of constraint GP k, likelihood noise included (GPModel.predict's convention), clipped as the acquisitions clip
 * theirs.  Everything is carried as log F = sum_k log Phi(z_k), summed in index order on every route; a location 45 sigma inside
 * the infeasible side has a finite log F and a finite gradient  sum_k lambda(z_k) (-dm_k - z_k ds_k) / s_k,  lambda = phi / Phi
 * formed in log space.
 *
 * A constraint handle is an ordinary gp_t: a fitted exact model (gp_fit) that holds neither a sparse fit nor an ensemble, on the
 * scored handle's device with the same D, P = 1 and no output warp, not the scored handle itself, every handle once.  Its
 * N, kernel, Gower set-up and mean function are its own.  GP_ERR_STATE: a handle that is not fitted; GP_ERR_ARG: everything
 * else, K outside 1 .. GP_FEAS_MAX, a c_std that is not positive and finite, a non-finite bound or c_mean.  No pointer to a
 * constraint handle is kept after a call returns.
 *
 * gp_feas_table caches log F over gp's resident candidates (GP_ERR_STATE without gp_set_data / gp_set_candidates; gp's own fit is
 * not needed).  For each constraint in turn gp's table is copied, device to device, into that handle's resident candidates --
 * AFTERWARDS THE CONSTRAINT HANDLE'S RESIDENT TABLE IS gp's, its cached posterior that table's --, the handle's table posterior
 * runs with the likelihood noise, and log Phi is added to gp's cache.  The cache is a snapshot: refitting or destroying a
 * constraint handle afterwards leaves it as it is (a new call refreshes it); gp_set_candidates / gp_set_candidates_kumar on gp,
 * gp_set_data with another D, and K = 0 (which takes null arguments) drop it.
 * gp_feas_info: *K constraints and *M rows of the cache, both 0 when there is none.  gp_feas_get_table: logF [M]; GP_ERR_STATE
 * without a cache.
 *
 * GP_ACQ_TIMES_FEAS in the `type` of gp_acq, gp_acq_argbest, gp_acq_topk, gp_acq_lp and gp_acq_lp_argbest multiplies the negated
 * scores by F behind the base rule -- ahead of the division of GP_ACQ_PER_COST and ahead of the penaliser's log transform, so a
 * penalised table scores EI F.  GP_ERR_ARG: LCB (its sign makes a product meaningless), no cache or one of another table size,
 * GP_ACQ_POF without the flag.  Every other entry refuses both: the table gradient entries, gp_acq_rows, the sparse, ensemble,
 * entropy-search, group and comm entries.
 *
 * gp_feas_rows: logF [M] and, when dlogF is given, its x-gradient [M, D] at M >= 1 locations Xs [M, D], through the constraint
 * handles' fused rows passes in groups of up to 8 locations (passes of 4 where M D > 128 doubles).
 * gp_acq_rows_feas: the acquisition optimiser's call.  Per pass: the scored handle's fused pass (type: GP_ACQ_EI, GP_ACQ_MPI or
 * GP_ACQ_POF, with GP_ACQ_TIMES_FEAS implied and GP_ACQ_PER_COST allowed; likelihood noise included), each constraint handle's
 * fused pass (gradients when dout is given), the fold  neg <- neg F, dneg <- F (dneg + neg dlogF)  into the scored handle's
 * result block, the cost division where asked for, then ONE drain -- no host round trip in between.  A handle that cannot take
 * the fused route (gp_rows_stats: option small_m, M D too wide, the inverse factor's build policy) goes through
 * gp_set_candidates and its table posterior instead -- its results stay on the device and are folded from there, and its
 * resident table is the group's locations afterwards (for gp that drops the cache of gp_feas_table).  There is no penaliser.
 *
 * gp_fmin_rows: gp_fmin's quantity -- y_i - (noise + 1e-8 + jitter) alpha_i over the raw targets -- minimised over the listed
 * training rows (the feasible ones); with every row listed it is gp_fmin bit for bit.  GP_ERR_ARG: n < 1, a row outside [0, N). */
int gp_feas_table(gp_t *gp, gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std);
int gp_feas_info(gp_t *gp, int *K, int64_t *M);
int gp_feas_get_table(gp_t *gp, double *logF);
int gp_feas_rows(gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std, const double *Xs,
                 int64_t M, double *logF, double *dlogF);
int gp_acq_rows_feas(gp_t *gp, gp_t *const *cons, int K, const double *bound, const double *c_mean, const double *c_std,
                     const double *Xs, int64_t M, int type, double par, double fmin, double y_mean, double y_std, double *out,
                     double *dout);
int gp_fmin_rows(gp_t *gp, const int64_t *rows, int64_t n, double *fmin);

/* ---- max-value entropy search (Wang & Jegelka, ICML 2017), mirrored for a minimum ----------------------------------------------
 * MES scores a location by the information its evaluation carries about the VALUE y* of the global minimum.  Given K samples
 * y*_0 .. y*_{K-1} of it (un-normalised, as fmin is) the score is a closed form of the posterior at the location: with m = mean
 * y_std + y_mean and s = sqrt(max(var y_std^2, 1e-10)) as every rule here forms them,
 *     g_k = (m - y*_k) / s,   h(g) = g lambda(g) / 2 - log Phi(g),   alpha = (1 / K) sum_k h(g_k),
 *     h'(g) = -(lambda / 2) (1 + g^2 + g lambda),   d alpha / dm = (1 / K) sum_k h'(g_k) / s,
 *     d alpha / ds = -(1 / K) sum_k h'(g_k) g_k / s,
 * lambda = phi / Phi formed in log space.  At and below g = -20 those forms cancel (h ~ log|g| between two terms of size g^2 / 2,
 * lambda's exponent likewise, the bracket of h' -> 2 / g^2), and h, lambda and the bracket come from the asymptotic series of Phi
 * instead: h and h' are good to a few 1e-15 relative at every g <= -20, finite where Phi underflows.  The three sums run over k = 0 .. K-1 in index order on every route, then are divided by K.  The
 * entries return -alpha and -d alpha / dx, the x-gradient assembled as for EI, LCB and MPI.
 *
 * gp_mes_set copies K samples into a buffer of the context's own (no caller pointer is kept); K = 0 clears (ystar may then be
 * NULL).  GP_ERR_ARG: K outside 0 .. GP_MES_MAX_K, a null pointer with K > 0, a sample that is not finite.  It touches neither the
 * fit nor any posterior cache, and the samples survive gp_fit, gp_set_params, gp_set_data and gp_set_candidates: they are the
 * caller's numbers in the caller's units, and keeping them current is the caller's business.
 * gp_mes_info: *K = samples resident, 0 when there are none.
 *
 * GP_ACQ_MES as the `type` of gp_acq, gp_acq_grad, gp_acq_argbest, gp_acq_topk, gp_acq_lp, gp_acq_lp_grad, gp_acq_lp_argbest and
 * gp_acq_rows (fused narrow and wide passes -- instances of the finishing kernel of their own --, the batched fallback, with or
 * without the penaliser) scores the rule over the resident samples; `par` and `fmin` are ignored.  GP_ACQ_PER_COST is allowed with
 * it (MES >= 0 is a gain, as EI is).  GP_ERR_STATE: no samples resident.  GP_ERR_ARG: GP_ACQ_TIMES_FEAS with it.  Every other
 * entry -- gp_acq_rows_feas, the sparse, ensemble, entropy-search, group and comm entries -- refuses it as an unknown acquisition.
 * Without a MES call every kernel is launched as before and returns the same bits.
 *
 * Sampling y* (the Gumbel approximation of the paper): over the M resident candidates with independent marginals
 *     log S(y) = log Pr[y* > y] ~ sum_i log Phi((m_i - y) / s_i).
 * gp_mes_logsurv: out[g] = that sum at the G trial values y [G], 1 <= G <= GP_MES_MAX_G, over the table posterior with
 * (include_noise = 1) or without the likelihood noise -- the sampler wants the latent one, y* being the minimum of f; it runs the
 * table posterior first where the cache does not hold it with that noise, and a scoring call afterwards re-runs its own (the cache
 * is keyed by the noise).  One pass over the table, each row's (m, s) loaded once for all G values.  The order of the sum is fixed
 * by ONE constant: chunks of 256 rows in row order, inside a chunk the four waves' fixed trees added in wave order, the chunks in
 * order; no atomics.  out[g] depends on y[g] and the table alone -- the same bits whatever G is and wherever the value stands --
 * and repeated calls are bitwise equal.
 * gp_mes_bracket: *lo = min_i (m_i - nsig s_i), *hi = min_i (m_i + nsig s_i), reduced on the device, every operation rounded on
 * its own (NumPy's bits on the same posterior).  With nsig = 8, S rounds to 1 at *lo and is below 1e-15 at *hi: a bracket for
 * every quantile.
 * Both need a fit and resident candidates (GP_ERR_STATE) and P = 1; GP_ERR_ARG: a null pointer, G out of range, a trial value,
 * y_mean or nsig that is not finite, nsig < 0, a y_std that is not positive and finite. */
int gp_mes_set(gp_t *gp, const double *ystar, int K);
int gp_mes_info(gp_t *gp, int *K);
int gp_mes_logsurv(gp_t *gp, int include_noise, double y_mean, double y_std, const double *y, int G, double *out);
int gp_mes_bracket(gp_t *gp, int include_noise, double y_mean, double y_std, double nsig, double *lo, double *hi);

/* ---- posterior paths: samples of the posterior FUNCTION by pathwise conditioning ----------------------------------------------
 * (Wilson et al., "Efficiently sampling functions from Gaussian process posteriors", ICML 2020.)  A path is
 *     f_s(x) = a sum_j w_js cos(omega_j^T x + b_j)  +  sum_n k(x, X_n) V_ns,       a = sqrt(2 variance / F),
 *     V_s = (K + d I)^-1 (y - Phi(X) w_s - eps_s),   eps_s = sqrt(d) z_s,   Phi(X)_nj = a cos(omega_j^T X_n + b_j),
 * d = noise + 1e-8 + jitter: the whole diagonal the resident factor carries, so that the update is exact for that factor.  The
 * first term is a random-Fourier-feature draw from the prior, the second an exact update through the factor of the fit: whatever F
 * is, f_s(X_i) = y_i - eps_si - d V_is.  Scope: the exact model with P = 1 and a Euclidean RBF, Matern-5/2, Matern-3/2 or
 * Exponential covariance, ARD or not.  Refused before anything is launched or changed: a Gower model (no spectral density,
 * GP_ERR_ARG), P != 1 (GP_ERR_ARG), a resident mean function or an output warp (GP_ERR_STATE), no fit (GP_ERR_STATE).
 *
 * gp_paths_set: S paths (1 .. GP_PATHS_MAX_S) of F features (1 .. GP_PATHS_MAX_F) from draws that do not depend on the
 * hyper-parameters: omega_unit [F, D] frequencies of the unit-lengthscale kernel, phase [F] in [0, 2 pi), w [S, F] and z_eps [S, N]
 * standard normals.  The library scales them from the RESIDENT parameters -- omega_jd = omega_unit_jd / lengthscale_d, a from the
 * variance, eps from d -- forms Phi(X) w (cos tiles in LDS against the fp64 matrix cores), the residuals, and V by the two
 * substitutions against the resident factor that alpha takes; nothing is factored.  S = 0 clears (the pointers may be NULL).
 * GP_ERR_ARG: S or F out of range, a null pointer, a draw that is not finite.  The paths belong to the factor: gp_fit,
 * gp_set_params, gp_set_data, gp_append and everything else that drops or grows it drop them, and the entries below then return
 * GP_ERR_STATE.  gp_paths_info: *S and *F of the resident paths, 0 and 0 when there are none.
 *
 * Values come back de-normalised, y_std f_s + y_mean (y_std positive and finite, y_mean finite, else GP_ERR_ARG).
 * gp_paths_table: out [S, M] (path-major), every resident path over the M resident candidates (gp_set_candidates; GP_ERR_STATE
 * without).  One kernel for a table that fills the chip by its rows alone, the kernel and a short summing launch otherwise (below):
 * tiles of K(x_i, X_n) are formed in LDS and contracted with V on the fp64 matrix cores, the feature term in the same kernel;
 * K(Xs, X) is never stored.  Per (path, candidate) the sum runs over n in tile order and over j in index order; a
 * table of few rows is also cut into chunks of training rows -- a function of (M, N) alone -- whose sums a second launch adds in
 * chunk order, so that it still fills the chip (scratch: (chunks + 1) S M doubles).  No atomics, the same bits whatever S is.
 * A workgroup of the kernel needs 8 (2 * 64 (D + 1) + 32 D + 2560 + 36 Spad) bytes of LDS, Spad = S rounded up to 16 -- a limit
 * JOINT in D and S: 121856 bytes at D = 64 and S = 64, inside the 163840 of gfx950, so every accepted (D, S) fits there; on a
 * device that gives a workgroup less, gp_paths_table and gp_paths_argbest return GP_ERR_ARG (the message names D, S and both byte
 * counts) before anything is launched.
 * gp_paths_argbest: idx [S], val [S]: per path the best row of that table (sense -1 minimum, +1 maximum; the lowest index among
 * ties), reduced on the device in one launch sequence for all paths.
 * gp_paths_rows: M <= 8 locations Xs [M, D] by value, row i on path path[i] (0 <= path[i] < S): out [M] and, when dout is given,
 * the x-gradient dout [M, D] = y_std (sum_n dk(x, X_n)/dx V_n - a sum_j w_j omega_j sin(omega_j^T x + b_j)).  The locations
 * travel in the kernel arguments, as many per pass as M D <= 128 coordinates allow -- all eight up to D = 16, two at D = 64 --
 * as in every rows entry; a pass is one launch and one synchronisation: partial sums over chunks of 256 training rows / features
 * with one writer each, combined in chunk order by the last workgroup to arrive, into a pinned block.  A row's bits depend on
 * neither the other rows, nor their paths, nor the pass it rides in.  Exponential at a coincident training point contributes 0 to
 * the gradient (the _inv_dist convention of every gradient here). */
#define GP_PATHS_MAX_S 64   /* paths resident at a time */
#define GP_PATHS_MAX_F 4096 /* random Fourier features of the prior term */
#define GP_PATHS_MAX_ROWS 8 /* locations per gp_paths_rows call */
int gp_paths_set(gp_t *gp, int S, int F, const double *omega_unit, const double *phase, const double *w, const double *z_eps);
int gp_paths_info(gp_t *gp, int *S, int *F);
int gp_paths_table(gp_t *gp, double y_mean, double y_std, double *out);
int gp_paths_argbest(gp_t *gp, double y_mean, double y_std, int sense, int64_t *idx, double *val);
int gp_paths_rows(gp_t *gp, const double *Xs, int M, const int *path, double y_mean, double y_std, double *out, double *dout);

/* ---- joint (batch) expected improvement qEI -----------------------------------------------------------------------------------
 * (Ginsbourger, Le Riche & Carraro 2010; Wang, Clark, Liu & Frazier 2016; Wilson, Hutter & Deisenroth, NeurIPS 2018.)  A batch of
 * q locations is scored as a whole,
 *     qEI(x_1 .. x_q) = E[max(0, max_j (fmin - par - y_j))],
 * over their JOINT posterior, by Monte Carlo with fixed base samples: y_s = m + C z_s, C C^T = Sigma (lower, rows in the caller's
 * order), z_s the first q entries of row s of Z; I_sj = fmin - par - y_sj, j*(s) = argmax_j I_sj (the lowest j on a tie), sample
 * s active when I_{s j*} > 0, qEI = (1 / S) sum_active I_{s j*}.  With Z fixed this is a deterministic function of the q D
 * coordinates with the gradient
 *     d qEI / d x_i = mbar_i dm_i/dx_i + sum_j A_ij dk(x_i, x_j)/dx_i - J_i^T (sum_j A_ij beta_j),
 * mbar_j = -(1 / S) #{active s: j*(s) = j}, Cbar_jl = -(1 / S) sum_{active s, j*(s) = j} z_sl (l <= j), P = tril(C^T Cbar) with its
 * diagonal halved, Sigma_bar = sym(C^-T P C^-1), A = 2 Sigma_bar, beta_j = Ky^-1 k(X, x_j), J_i the [N, D] input Jacobian of
 * k(X, x_i).  The posterior is gp_predict_rows': m_i = k_i^T alpha, Sigma_ij = k(x_i, x_j) - w_i . w_j with w_i = L^-1 k_i, the
 * likelihood noise on the diagonal with include_noise; m and Sigma de-normalised (y_std m + y_mean, y_std^2 Sigma) before the
 * factorisation, as gp_acq_rows de-normalises mean and variance (no clip: a variance that is not positive ends the call, below).
 *
 * gp_qei_set: Z [S, q] standard normals, 1 <= S <= GP_QEI_MAX_S, 1 <= q <= GP_QEI_MAX_Q, made resident (a copy).  They belong to
 * no fit: gp_fit, gp_set_params, gp_set_data and gp_append leave them (common random numbers across refits); they go with the
 * handle.  GP_ERR_ARG: a null pointer, S or q out of range, a sample that is not finite.  gp_qei_info: *S and *q resident, 0 and 0
 * without.  gp_qei_stats: gp_qei_rows calls answered since the context was created, and those of them with a gradient
 * (gp_rows_stats and gp_rows_pass_stats count what they counted: these calls do not move them).
 *
 * gp_qei_rows: Xq [q, D] by value, q up to the resident q (a smaller q reads the leading q columns of Z: the same bits as a
 * handle given Z[:, :q]).  out[0] = -qEI and, when dout is given, dout [q, D] = -d qEI / d x (the sign of gp_acq / gp_acq_grad);
 * mean [q] and cov [q, q] (row-major, de-normalised, the matrix that was factored) when given; dout, mean, cov may be NULL.  The
 * diagonal of cov at y_std = 1 is gp_predict_rows' variance of a value call, bit for bit.  Launches: the fused rows path's forward
 * pass over the inverse factor for all q locations at once (pass layouts 1, 4 and 8 as there); the Gram of the w_i per 64
 * training rows; ONE workgroup that assembles m and Sigma, factors it, walks the samples (thread t takes s = t, t + 256, ... in
 * order, the threads' sums are added in thread order within groups of 64, the groups in order) and forms mbar and A; for a gradient the rows path's backward pass and a
 * closing pass over the training points that mixes A into the beta_j -- t_i = sum_j A_ij beta_j, so the q x q adjoint costs no
 * further pass over the factor -- and whose last workgroup writes the results into the pinned block.  A value call skips the
 * last two.  No copy commands either side of the launches, no atomics but the arrival counter: repeated calls are bitwise equal,
 * and the value has the same bits with and without dout.  The inverse factor is built at the first call after a fit where it
 * does not exist.  Always true fp64 (option "emulate_fp64" does not reach it).
 * Returns: 0; a POSITIVE value r when pivot r (1-based row of Sigma, caller's order) is not positive or not finite -- coincident
 * locations without noise: nothing is written; GP_ERR_STATE: no fit, no resident samples, P != 1, a Gower kernel, an output warp
 * or a mean function in force; GP_ERR_ARG: a null gp / Xq / out, q outside 1 .. resident q, q D > 128 coordinates, a location,
 * par, fmin or y_mean that is not finite, a y_std that is not positive and finite.  A refused call launches and changes nothing. */
#define GP_QEI_MAX_S 4096 /* base samples resident at a time */
#define GP_QEI_MAX_Q 8    /* locations of a batch */
int gp_qei_set(gp_t *gp, const double *Z, int S, int q);
int gp_qei_info(gp_t *gp, int *S, int *q);
int gp_qei_stats(gp_t *gp, int64_t *calls, int64_t *grad_calls);
int gp_qei_rows(gp_t *gp, const double *Xq, int q, int include_noise, double par, double fmin, double y_mean, double y_std,
                double *out, double *dout, double *mean, double *cov);

/* ---- multi-objective: expected hypervolume improvement (Emmerich et al. 2011; Yang et al. 2019) ---------------------------------
 * K = 2 or 3 objectives, all minimised, each modelled by an exact GP on a handle of its own (independent objectives).  With the
 * region of (-inf, r] that the observed Pareto front does not dominate cut into C axis-parallel cells [l_c, u_c] (l_ck = -inf
 * allowed),
 *     EHVI(x) = sum_c prod_k (Psi_k(u_ck) - Psi_k(l_ck)),   Psi_k(c) = s_k (z Phi(z) + phi(z)),  z = (c - m_k) / s_k,  Psi_k(-inf) = 0,
 * m_k / s_k objective k's predictive mean and standard deviation at x, un-normalised by (y_mean[k], y_std[k]) and clipped at
 * 1e-10 as every rule here, likelihood noise included.  Psi is EI with incumbent c and no jitter: d Psi / dm = -Phi, d Psi / ds = phi.
 *
 * The decomposition is the caller's (multi_objective.nondominated_cells builds it) and lives on the SCORED handle, objective 0:
 * gp_ehvi_set copies it to the device.  levels: objective k's nlev[k] coordinates, the K arrays behind each other; entry 0 of each
 * is -inf (read as such whatever is stored there), the others finite and increasing, the last one r_k.  cell_lo / cell_hi [C, K]:
 * indices into objective k's levels, lo < hi.  The values are in raw objective units, so the state survives refits; K = 0 and
 * gp_destroy drop it.  GP_ERR_ARG: K outside 2 .. GP_EHVI_MAX_OBJ (0 clears), nlev[k] outside 2 .. GP_EHVI_MAX_LEVELS, C outside
 * 1 .. GP_EHVI_MAX_CELLS, levels not finite or not increasing above index 0, an index out of range, lo >= hi.
 * gp_ehvi_info: *K and *C, both 0 when there is none.
 *
 * `others` are the K - 1 handles of objectives 1 .. K - 1; y_mean / y_std [K] the output normalisers, objective 0 first.
 * GP_ERR_STATE: no gp_ehvi_set, a handle without a fit (the table entries: no resident candidates on gp).  GP_ERR_ARG: a K that
 * differs from the state's, a handle listed twice or equal to gp, another device or another D, P != 1, a sparse fit, an ensemble or
 * an output warp on any handle, a y_mean that is not finite, a y_std that is not positive and finite.
 *
 * gp_ehvi_table: -EHVI over gp's resident candidates into gp's score table, and into out [M] when given.  The table goes to the
 * other handles device to device (it is their resident table afterwards, as after gp_feas_table); K table posteriors, then ONE
 * launch with one workgroup per row.  gp_ehvi_argbest / gp_ehvi_topk: the same, then the selector of gp_acq_argbest /
 * gp_acq_topk (lowest index among equal scores; sense -1 picks the largest EHVI).
 * gp_ehvi_rows: out [M] = -EHVI and, when dout is given, dout [M, D] = -d EHVI / dx at M >= 1 locations Xs [M, D], the
 * acquisition optimiser's call.  Groups of up to eight locations, passes of four where M D > 128; per pass every handle's fused
 * one-location pass, the fold (one workgroup per location), then the owners' waits: one drain, no host round trip in between.  A
 * handle that cannot take the fused route goes through its table posterior over the group (its resident table is the group's
 * locations afterwards) and is folded from its device buffers.
 * A location's bits do not depend on its company, and the value is the same bits with and without dout (the posterior behind a
 * value-only call is the gradient call's, backward launch included; the table entry's scores agree with it to rounding, and bit
 * for bit when both fold the same posterior):
 * one device routine serves both kernels -- the K L levels' Psi / Phi / phi once into LDS, thread t takes cells t, t + 256, ... in
 * order, the threads' sums meet in a reduction of fixed shape, no atomics. */
#define GP_EHVI_MAX_OBJ 3
#define GP_EHVI_MAX_LEVELS 256
#define GP_EHVI_MAX_CELLS 32768
int gp_ehvi_set(gp_t *gp, int K, const double *levels, const int *nlev, const int *cell_lo, const int *cell_hi, int C);
int gp_ehvi_info(gp_t *gp, int *K, int *C);
int gp_ehvi_table(gp_t *gp, gp_t *const *others, int K, const double *y_mean, const double *y_std, double *out);
int gp_ehvi_argbest(gp_t *gp, gp_t *const *others, int K, const double *y_mean, const double *y_std, int sense,
                    const int64_t *exclude, int nex, int64_t *idx, double *val);
int gp_ehvi_topk(gp_t *gp, gp_t *const *others, int K, const double *y_mean, const double *y_std, int sense, int k, int64_t *idx,
                 double *val);
int gp_ehvi_rows(gp_t *gp, gp_t *const *others, int K, const double *y_mean, const double *y_std, const double *Xs, int64_t M,
                 double *out, double *dout);

/* ---- knowledge gradient (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011) ---------------------------------------------
 * The expected decrease of the minimum of the posterior mean after one more (noisy) observation at x, the minimum taken over a
 * resident discretisation set X_A = {a_0 .. a_{A-1}} and x itself.  With w = L^-1 k(X, x), v = kss - |w|^2, sigma^2 the likelihood
 * variance gp_predict's include_noise adds, everything de-normalised by y_std (the shift y_mean cancels):
 *     v'  = max(y_std^2 v, 1e-10)                                   (the floor of gpmodel.py:99, as gp_es_acq applies it)
 *     sd  = sqrt(v' + y_std^2 sigma^2)
 *     a_i = y_std mu(a_i),  b_i = y_std^2 (k(x, a_i) - V_A[i] . w) / sd,   i < A;      a_A = y_std mu(x),  b_A = v' / sd
 *     a*  = min_i a_i (lowest index on a tie),  a~_i = a_i - a* >= 0
 *     KG(x) = -E_Z[min_i (a~_i + b_i Z)] = -sum_i (a~_i p_i + b_i q_i),   p_i = Phi(hi_i) - Phi(lo_i),  q_i = phi(lo_i) - phi(hi_i)
 * [lo_i, hi_i] the interval of z on which line i is the lowest (empty for dominated lines; of lines identical to the bit the lowest
 * index owns it), found in interval form: line i intersects the half-lines (b_i - b_j) z <= a~_j - a~_i over all j.  p_i comes from
 * erfc on the side of the tail.  Gradient, j* = argmin_i a_i:
 *     dKG/dx = ([j* = A] - p_A) y_std dmu(x)/dx - sum_i q_i db_i/dx
 *     db_i/dx = y_std^2 (dk(x, a_i)/dx - J(x)^T beta_{a_i}) / sd - b_i dsd / sd  (i < A),   db_A/dx = dv' / sd - b_A dsd / sd
 *     dv' = -2 y_std^2 J(x)^T beta_x (0 where the floor holds),  dsd = dv' / (2 sd),  beta_{a_i} = L^-T V_A[i],  beta_x = L^-T w
 * J(x) the [N, D] input Jacobian of k(X, x), 0 where the distance is exactly 0.
 *
 * gp_kg_set_points: Xa [A, D] becomes resident with V_A = L^-1 K(X, Xa) (a padded 256 x Npad block of its own) and the points'
 * latent means; mu [A], when given, receives them un-normalised (mean y_std + y_mean).  Entropy search's representers and their
 * bits are left alone, and gp_es_set_representers leaves the points: both may be resident.  The resident candidates stay; their
 * cached posterior is dropped.  The points belong to the fit: everything that drops the representers drops them.  gp_kg_info:
 * *A resident, 0 without.
 * gp_kg_acq: out [M] = +KG over the resident candidates.  Per chunk of the candidate solve C = K(Xs, Xa) - (K(Xs, X) L^-T) V_A^T,
 * the GEMM of gp_es_acq against V_A, then one workgroup per candidate.  gp_kg_acq_argbest / gp_kg_acq_topk: the selector of
 * gp_acq_argbest / gp_acq_topk over that vector (sense +1 picks the largest KG; lowest index among equal scores).
 * gp_kg_rows: M >= 1 locations Xs [M, D] by value; out [M] = -KG and, when dout is given, dout [M, D] = -dKG/dx (the sign of
 * gp_acq / gp_acq_grad).  For M <= option "small_m" (8) locations that fit the fused rows path (pass layouts 1, 4 and 8, the
 * build policy of the inverse factor as for gp_acq_rows; a gradient call always takes the factor) a pass is the forward launch
 * over L^-1, the shares of V_A w per 256 training rows, a scoring launch of one workgroup per location that forms the C's, scores
 * and leaves p, q and the adjoint coefficients, and for a gradient: a kernel that mixes them into the backward pass's right-hand
 * sides, w' = cw w + sum_i cv_i V_A[i] -- by linearity L^-T w' carries beta_x and
 * every beta_{a_i}, so L^-1 is read twice as in gp_acq_rows and no B_A = L^-T V_A is kept --, the rows path's backward pass, and a
 * closing pass over the training points.  Results and ticket go into the pinned block: no copy commands either side.  Larger M,
 * or a shape the fused path refuses, takes the two table calls, values only: a dout there is GP_ERR_ARG.  The routes agree to
 * rounding (tests: 1e-9).  On the fused path a location's value and gradient are the same bits whatever its slot and its company,
 * repeated calls are bitwise equal, and the value is the same bits with and without dout.  Fixed summation order, no atomics but
 * the arrival counter.  Always true fp64 ("emulate_fp64" covers the candidate solve of the table as for gp_predict).
 * GP_ERR_STATE: no fit, no resident points (scoring), P != 1, a sparse fit, an ensemble, an output warp, a mean function or a Gower
 * kernel in force.  GP_ERR_ARG: A outside 1 .. GP_KG_MAX_A, null pointers, inputs that are not finite, a y_std that is not positive
 * and finite.  A refused call launches and changes nothing. */
#define GP_KG_MAX_A 256
int gp_kg_set_points(gp_t *gp, const double *Xa, int A, double y_mean, double y_std, double *mu);
int gp_kg_info(gp_t *gp, int *A);
int gp_kg_acq(gp_t *gp, double y_std, double *out);
int gp_kg_acq_argbest(gp_t *gp, double y_std, int sense, int64_t *idx, double *val);
int gp_kg_acq_topk(gp_t *gp, double y_std, int sense, int k, int64_t *idx, double *val);
int gp_kg_rows(gp_t *gp, const double *Xs, int64_t M, double y_std, double *out, double *dout);

/* ---- noisy expected improvement (Letham, Karrer, Ottoni & Bakshy 2019) ---------------------------------------------------------------
 * EI averaged over S draws ("fantasies") of the noiseless function values at the training inputs.  Two handles on one device hold
 * the same X, kernel family, variance and lengthscales: the MODEL is the noisy fit, factor L L^T = Ky = K + d I with
 * d = noise + 1e-8 + jitter and normalised targets y; the TWIN is a near-noiseless fit of the same kernel, L0 L0^T = K0 = K + d0 I,
 * d0 = noise0 + 1e-8 + jitter0 (its Y is not read).  The latent f has prior covariance K0 and y = f + eps, eps ~ N(0, (d - d0) I),
 * so that the model's covariance is exactly Ky.  Matheron's rule, from standard normals Z, E [S, N] (row s is fantasy s):
 *     g_s = L0 z_s,   r_s = y - g_s - sqrt(d - d0) e_s,   V_s = Ky^-1 r_s,
 *     F_s = y - sqrt(d - d0) e_s - (d - d0) V_s   (= g_s + K0 Ky^-1 r_s),   a_s = K0^-1 F_s,   fstar_s = min_i F_is.
 * At a location x: k = k(X, x), w = L0^-1 k, m_s = k . a_s, and s the twin's predictive standard deviation as gp_acq_rows forms it
 * (variance kss - |w|^2 + noise0, times y_std^2, floored at 1e-10, root floored at 1e-10).  mu_s = y_std m_s + y_mean,
 * t_s = y_std fstar_s + y_mean, u_s = (t_s - par - mu_s) / s:
 *     NEI(x) = (1 / S) sum_s s (u_s Phi(u_s) + phi(u_s))                              (s = 0 .. S - 1 in index order)
 *     dNEI/dx = -y_std J^T (A0 p) + c ds/dx,   p_s = Phi(u_s) / S,   c = (1 / S) sum_s phi(u_s),   A0 = [a_1 .. a_S]
 * J the [N, D] input Jacobian of k(X, x) (0 where the distance is exactly 0), ds/dx = -(y_std^2 / s) J^T L0^-T w, 0 where the
 * floor holds.
 *
 * gp_nei_set(twin, model, S, Z, E): the state becomes resident on the TWIN -- A0 and U = L0^-1 F ([64, Npad] each, fantasy-major),
 * F, fstar, d and d0.  Nothing is factored.  g = L0 z is one streaming read of L0's lower triangle by a kernel of its own (dA's
 * upper tiles hold what the factorisation left there, so the GEMM does not apply); the residual and F are one kernel; the column
 * minima a fixed-order reduction; the four substitutions are the two alpha takes, S right-hand sides each, against either factor
 * (the model's inverted diagonal panels are built where they were not: nothing else of the model changes).  Each fantasy is its own
 * dot products: the leading S columns of a larger draw give the same bits.  S = 0 clears the state (model, Z, E may be NULL).
 * The state belongs to both factors: whatever drops or grows the twin's factor drops it, and every gp_nei_* entry returns
 * GP_ERR_STATE once the model has been refitted, appended to, given new data or parameters, or destroyed.
 * gp_nei_info: *S resident (0 without), *d_model and *d_twin (any may be NULL).  gp_nei_get: F [S, N] and fstar [S], normalised
 * (either may be NULL).
 * gp_nei_table: out [M] = +NEI over the twin's resident candidates: the variance from the candidate solve of gp_predict, the S
 * means from gp_paths_table's fused kernel-build-and-product with A0 in V's place and no feature term (K(Xs, X) is not stored),
 * then one scoring launch.  gp_nei_argbest / gp_nei_topk: the selector of gp_acq_argbest / gp_acq_topk over that vector (sense +1
 * picks the largest NEI; lowest index among equal scores).  The LDS of the product is joint in D and S as for gp_paths_table: a
 * shape that does not fit is GP_ERR_ARG naming both byte counts.
 * gp_nei_rows: M >= 1 locations by value; out [M] = -NEI and, when dout is given, dout [M, D] = -dNEI/dx.  For M <= option
 * "small_m" (8) locations that fit the fused rows path (layouts 1, 4, 8; the inverse factor's build policy as for gp_acq_rows, a
 * gradient call always takes the factor) a pass is: the forward launch over L0^-1; the shares of k . a_s and |w|^2 per 256
 * training rows, one writer each; a scoring launch of one workgroup per location that adds the shares in order, scores the S
 * fantasies and leaves p and c; and for a gradient: the mix w' = -(c y_std^2 / s) w - y_std sum_s p_s U_s into the backward
 * pass's right-hand sides -- L0^-T w' is the whole adjoint, since L0^-T U_s = a_s --, the rows path's unchanged backward pass and
 * the closing pass over the training points whose last workgroup writes the pinned block.  L0^-1 is read twice for a gradient,
 * once for a value, whatever S.  Other shapes take the table route, values only: a dout there is GP_ERR_ARG.  On the fused path
 * repeated calls are bitwise equal, the value has the same bits with and without dout, and a location has the same bits whatever
 * its slot, its company and its pass layout.  No atomics but the arrival counter; always true fp64.
 * gp_nei_stats (route checks; any pointer may be NULL): *linv_builds how often the handle's inverse factor was built since
 * gp_create (once per fit that a rows call follows), *pass_launches the kernels the last pass of the last gp_nei_rows call put on
 * the stream and *pass_reads how many of them read L0^-1 -- 3 and 1 for a value call, 6 and 2 for a gradient call, 0 and 0 where
 * the call took the table route.  Counted where the kernels are launched.
 * GP_ERR_STATE: either handle unfitted, P != 1, a Gower kernel, a mean function, an output warp, a Laplace or sparse fit or an
 * ensemble on either handle, no resident state (scoring), the model changed since gp_nei_set.  GP_ERR_ARG: null pointers,
 * different devices, N, D, kernel, ARD flag, variance, lengthscales or X (compared on the device), d <= d0, S outside
 * 0 .. GP_NEI_MAX_S, a draw or a location that is not finite, a normaliser that is not usable.  A refused call launches and changes
 * nothing. */
#define GP_NEI_MAX_S 64
#define GP_NEI_MAX_ROWS 8
int gp_nei_set(gp_t *twin, gp_t *model, int S, const double *Z, const double *E);
int gp_nei_info(gp_t *twin, int *S, double *d_model, double *d_twin);
int gp_nei_get(gp_t *twin, double *F, double *fstar);
int gp_nei_stats(gp_t *twin, int64_t *linv_builds, int *pass_launches, int *pass_reads);
int gp_nei_table(gp_t *twin, double par, double y_mean, double y_std, double *out);
int gp_nei_argbest(gp_t *twin, double par, double y_mean, double y_std, int sense, int64_t *idx, double *val);
int gp_nei_topk(gp_t *twin, double par, double y_mean, double y_std, int sense, int k, int64_t *idx, double *val);
int gp_nei_rows(gp_t *twin, const double *Xs, int64_t M, double par, double y_mean, double y_std, double *out, double *dout);

/* ---- GP classification: Bernoulli likelihood, probit link, Laplace's approximation (api_laplace.hip) --------------------------
 * Rasmussen & Williams, Algorithms 3.1 and 5.1.  labels [N] in {-1, +1} (anything else: GP_ERR_ARG); X and the kernel are the
 * context's (gp_set_data with P = 1 -- its Y is not read -- and gp_set_params, whose noise is ignored: K carries no noise and no
 * 1e-8).  With z = y f and n = phi(z) / Phi(z) the sites are log p = log Phi(z), g = y n, W = n (n + z) floored at 1e-20,
 * t = y (n (z^2 - 1) + 3 z n^2 + 2 n^3), n formed in log space.
 * gp_laplace_fit: Newton's iteration in a = K^-1 f from a = 0; per step the sites, B = I + W^1/2 K W^1/2 and its factorisation
 * (the one gp_fit takes at that N; no jitter ladder: B has eigenvalues >= 1), two triangular solves, one product K da; the step
 * is halved while psi(a) = -a.K a / 2 + sum log p decreases.  It stops when the accepted step is at most 1e-10 of max |a| or psi
 * has not moved by 1e-13 of its size twice in a row.  *logz = -a.f / 2 + sum log p - log|B| / 2, *logdet_b = log|B|, *iters and
 * *halvings the steps and halvings taken, *converged 1 (out-parameters may be NULL).  Returns 0; GP_LAPLACE_NOT_CONVERGED when
 * max_iter (1 .. GP_LAPLACE_MAX_ITER) steps did not suffice or the line search failed (30 halvings; gp_last_error says which);
 * another positive code when a pivot of B failed (non-finite inputs);
 * either way no fit is left.  On success the context is "Laplace-fitted": its factor is that of K + W^-1 (diag(W^-1/2) L), its
 * alpha is a, its noise 1, so gp_predict, gp_predict_rows, gp_predict_grad, the candidate tables, gp_feas_* and gp_acq_rows_feas
 * answer with the latent posterior -- with include_noise variance s^2 + 1, as p(y = 1 | x) = Phi(m / sqrt(1 + s^2)) takes it.
 * gp_set_data, gp_set_params and every regression fit clear the state (and put gp_set_params' noise back).  Refused on such a
 * context (GP_ERR_STATE): gp_append, gp_fmin, gp_fmin_rows, gp_lml_grad, gp_lml_grad_x, gp_get_dl_dk, gp_mean_set, gp_mean_grad,
 * gp_paths_set, gp_qei_rows, the knowledge-gradient and entropy-search entries, gp_mes_set / gp_mes_logsurv / gp_mes_bracket and
 * GP_ACQ_MES, gp_cost_set and GP_ACQ_PER_COST, gp_group_fmin and the gp_group_acq_* entries (gp_group_set_data, _set_params and
 * _fit clear the state), the batched fits, the sparse model's entries over a sparse fit (gp_sparse_fit itself clears the state)
 * and gp_comm_bcast_fit from such a root.  gp_kernel_matrix drops the state with the factor it overwrites.  The fit itself is refused
 * (GP_ERR_STATE) with P != 1, a Gower kernel, an output warp or a mean function.  Always true fp64; the same inputs give the
 * same bits.  Memory: one more Npad x Npad matrix (K) beside the factor's.
 * gp_laplace_fit_grad: the fit, then grad [1 + nls] = d logz / d (variance, lengthscale(s)) (nls = 1, or D with ard), implicit
 * part included: sum_ij G_ij dK_ij with G = (a a^T - R + u a^T + a u^T) / 2, R = (K + W^-1)^-1, s2 = diag(K - K R K) t / 2,
 * u = (I - R K) s2.  D beyond what the gradient pass's LDS takes: GP_ERR_ARG before the fit.
 * gp_laplace_info: steps, halvings and min / max of W of the last fit; gp_laplace_get_mode: f [N] at the mode and W [N] (either
 * may be NULL).  Both need a Laplace-fitted context (GP_ERR_STATE). */
#define GP_LAPLACE_MAX_ITER 1000
#define GP_LAPLACE_NOT_CONVERGED 1073741824
int gp_laplace_fit(gp_t *gp, const double *labels, int max_iter, double *logz, double *logdet_b, int *iters, int *halvings,
                   int *converged);
int gp_laplace_fit_grad(gp_t *gp, const double *labels, int max_iter, double *logz, double *logdet_b, int *iters, int *halvings,
                        int *converged, double *grad);
int gp_laplace_info(gp_t *gp, int *iters, int *halvings, double *wmin, double *wmax);
int gp_laplace_get_mode(gp_t *gp, double *f, double *W);

#ifdef __cplusplus
}
#endif
#endif /* GPHIP_H */
