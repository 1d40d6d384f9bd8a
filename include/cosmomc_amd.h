/* cosmomc_amd -- MI355X-native fast-parameter likelihood + MCMC step for CosmoMC.
 *
 * C ABI of libcosmomc_amd.so.  Plain pointers and sizes only; every device
 * pointer argument is a HIP device pointer (e.g. torch.Tensor.data_ptr() of a
 * cuda tensor), every stream a hipStream_t (NULL = default stream).
 * Errors are returned as negative codes plus a message (never an abort);
 * the message of the last failing call on a handle is cmbl_last_error().
 *
 * Reference interfaces replaced (SouthPoleTelescope/CosmoMC):
 *   cmbl_open            CMBLikelihood_Add tag dispatch + ReadDatasetFile/ReadIni
 *                        (source/CMB.f90:54-123, source/likelihood.f90:36-66,
 *                         source/CMB.f90:208-303 for PLIK_LITE)
 *   cmbl_info            TDataLikelihood metadata (source/GeneralTypes.f90:105-126):
 *                        nuisance params, cl_lmax(4,4), speed, name
 *   cmbl_derived_info / cmbl_derived_batch
 *                        DataLike%derivedParameters(Theory, DataParams) and its
 *                        '*' names (source/GeneralTypes.f90:504-512, 658-664, 774-776;
 *                        TSmica_planck_derivedParameters source/CMBlikes.f90:1324-1337)
 *   cmbl_loglike_batch   like%LogLike(CMB, Theory, DataParams) for W walkers at once
 *                        (source/CMB.f90:305-329; called from calclike.f90:380)
 *   cmbl_clik_compute_batch  clik_lnlike packing (source/cliklike.f90:129-170) routed
 *                        to the native kernel; returns +lnL like clik_compute
 *   cmbt_*               the calculator object's theory at a slow point, as a polynomial
 *                        response surface of D_l (the slot of source/Calculator_PICO.f90;
 *                        error = 1 outside the box -> logZero, calclike.f90:308-313)
 *   cmbt_set_derived / cmbt_derived_eval
 *                        the parameterization's derived parameters (TP_CalcDerivedParams,
 *                        source/CosmologyParameterizations.f90:189-272) as response surfaces,
 *                        and TP_NonBaseParameterPriors' hard cuts on them (:90-112)
 *   cmbs_*               BlockedProposer (source/propose.f90:53-298) + Metropolis
 *                        (source/MCMC.f90:119-335) + GetLogLike bounds/priors/temperature
 *                        (source/calclike.f90:82-151), batched over W independent chains
 */
#ifndef COSMOMC_AMD_H
#define COSMOMC_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMBL_LOGZERO 1e30          /* settings.f90:114 logZero */

enum {
    CMBL_OK = 0,
    CMBL_ERR_ARG = -1,             /* bad argument */
    CMBL_ERR_IO = -2,              /* dataset / data file unreadable */
    CMBL_ERR_FORMAT = -3,          /* dataset content invalid */
    CMBL_ERR_NUMERIC = -4,         /* covariance not positive definite, ... */
    CMBL_ERR_HIP = -5,             /* HIP runtime error */
    CMBL_ERR_UNSUPPORTED = -6      /* dataset type / option not implemented */
};

/* Theory layout: field pair f of Theory%Cls(i,j), i>=j with T=1,E=2,B=3,P=4,
 * f = i*(i-1)/2 + j - 1: TT=0 TE=1 EE=2 BT=3 BE=4 BB=5 PT=6 PE=7 PB=8 PP=9.
 * D_l = l(l+1)C_l/2pi in muK^2 (source/CosmoTheory.f90:25), indexed from l=0:
 *   dl[w*ld_walker + f*ld_field + l]. */
#define CMBL_NFIELDS 10

typedef struct cmbl cmbl_t;

/* tag -> likelihood class as CMBLikelihood_Add (source/CMB.f90:80-97):
 * "PLIK_LITE" native plik_lite (CMB.f90:30-329), "BKPLANCK" CMBlikes with the
 * BICEP/Keck/Planck foregrounds (CMB_BK_Planck.f90), "SPTPOL_TEEE" / "SPTPOL_BB"
 * the SPTpol TE/EE 2017 and BB 2019 likelihoods (CMB_SPTpol_TEEE_2017.f90,
 * CMB_SPTpol_BB_2019.f90; sptpol_blind_r is CMBL_ERR_UNSUPPORTED), "SMICA"
 * CMBlikes with the SMICA TT foreground, nuisance_params and
 * calibration_paramname (TSmica_planck, CMBlikes.f90:1262-1339; binned HL or
 * gaussian), "JLA" the JLA supernova likelihood (supernovae_JLA.f90; a
 * jla.dataset with the 16-column light-curve file and any of the six
 * covariance components, file names as written or relative to the dataset;
 * nuisance parameters alpha_JLA beta_JLA; JLA_marginalize = T and absdist_file
 * are CMBL_ERR_UNSUPPORTED, a matrix of the wrong size or a set number outside
 * 0..9 CMBL_ERR_FORMAT), "JLA_MARGE" the same dataset with JLA_marginalize = T
 * (supernovae_JLA.f90:235-252, 1207-1217): alpha and beta integrated over the
 * reference's fixed grid, options JLA_marge_steps (7; outside 0..16 is
 * CMBL_ERR_ARG), JLA_step_width_alpha (0.003) and JLA_step_width_beta (0.04; a
 * width <= 0 is CMBL_ERR_ARG) from the dataset or the overrides; no nuisance
 * parameters; V(alpha, beta)^-1 of every grid point is formed on the device at
 * open (cmbl_jla_marge_info); a point where V does not factor is dropped as the
 * reference drops it, none left or the two-scriptm assumption violated at a
 * point is CMBL_ERR_FORMAT (JLA_alpha_center and JLA_beta_center move the
 * grid's centre from the reference's constants: an extension, for tests),
 * "WL" a DES-format weak-lensing and galaxy-clustering dataset (wl.f90; see
 * cmbl_wl_info below for its theory row and options),
 * "SZ" the Planck SZ cluster counts (szcounts.f90; see cmbl_sz_info below for
 * its ini, theory row and options),
 * "MPK" a galaxy power-spectrum dataset of mpk.f90's format (sdss_lrgDR4.dataset)
 * and "WIGGLEZ" one redshift bin of wigglez.f90 (wigglez_nov11a.dataset, the
 * keys of the wigglez_common_dataset file as overrides; see cmbl_mpk_info below
 * for the theory row, the keys and the refusals),
 * "WMAP" CMBL_ERR_UNSUPPORTED (external library), any other tag a CMBlikes
 * dataset (CMBlikes.f90; like_approx HL or gaussian, binned, or exact,
 * unbinned: ExactChiSq CMBlikes.f90:967-979, up to 4 maps).
 * override_ini: "key = value" lines applied over the dataset file, as
 * cmb_dataset[TAG,key] = value (source/CMB.f90:71-74); may be NULL. */
int  cmbl_open(const char *tag, const char *dataset_path, const char *override_ini,
               cmbl_t **out, char *errbuf, size_t errlen);
void cmbl_close(cmbl_t *h);
const char *cmbl_last_error(const cmbl_t *h);

/* cl_lmax: 16 ints, cl_lmax[(i-1)*4 + (j-1)] = cl_lmax(i,j) (0 = unused).
 * speed: likelihood speed (-1 = slow default of TCMBLikelihood).
 * nuisance_names: space separated names from the calibration/nuisance
 * .paramnames (pointer owned by the handle). */
int  cmbl_info(const cmbl_t *h, int *n_nuis, int *cl_lmax, int *speed,
               const char **name, const char **nuisance_names);

/* Theory of a likelihood that reads no C_l: the doubles of one walker's theory
 * row, all in field 0 (dl[w * ld_walker + i], i = 0 .. len-1; ld_field unused).
 * JLA: its nsn distance moduli 5 log10((1+zhel_i)(1+zcmb_i) D_A(zcmb_i) / Mpc)
 * (supernovae_JLA.f90:1195-1199), its cl_lmax all zero.  0 for the CMB
 * likelihoods.  A calculator serves such a row with n_fields = 1, fields = {0},
 * lmax = len - 1. */
int  cmbl_theory_len(const cmbl_t *h);

/* "WL" (the DES-format weak-lensing and galaxy-clustering likelihood, wl.f90):
 * a walker's theory row is
 *     [h, omm, chis[nz], Hs[nz], D_growth[nz], P[nl][nz]]
 * (2 + 3 nz + nl nz doubles): h = H0/100, omm = omdm + omb, chis the comoving
 * distances and Hs the H(z) of the calculator at z_p (nz = num_z_p: the n(z)
 * file's rows + 2), D_growth = sqrt(P_lin(0.01, z_p) / P_lin(0.01, 0)), and
 * P[l * nz + j] the power calc_theory holds in `powers` (wl.f90:549-569) at
 * kh = (ls_cl[l] + 1/2) / (chis[j] h), z_p[j], 0 where kh is outside the
 * spectrum's range; nl = size(ls_cl).  The library uses the row as given.
 * Nuisance parameters in DataParams order (b, m, A, alpha, z0, DzL, DzS), named
 * by the dataset's nuisance_params file; option keys acc, lmax, ah_factor (read,
 * not applied), intrinsic_alignment_model = none | DES1YR, used_data_types,
 * num_gal_bins = 0, and wl_use_weyl as an override key (with gammat or wtheta
 * wanted: CMBL_ERR_UNSUPPORTED, as wl.f90:201-203).  Any key WL_ReadIni does
 * not read, and any measurements_format but DES, is CMBL_ERR_UNSUPPORTED and
 * named in the message.
 * cmbl_wl_info: dims[8] = nz, nl, size(ls_bessel), Limber columns, num_used,
 * first_theta_bin_used, num_z_bins, num_gal_bins.  cmbl_wl_arrays: ls_cl [nl],
 * ls_bessel, used_items [num_used][4] (type index, bin1, bin2, theta bin; all
 * 1-based); any pointer may be NULL.  CMBL_ERR_ARG for another likelihood. */
int  cmbl_wl_info(const cmbl_t *h, int *dims);
int  cmbl_wl_arrays(const cmbl_t *h, int *ls_cl, double *ls_bessel, int *used_items);

/* "SZ" (the Planck SZ cluster-counts likelihood, szcounts.f90, its 2D form
 * N(z, q)): the file opened is a small ini with cat_file, thetas_file,
 * skyfracs_file and ylims_file (the reference's data/SZ_*.txt, relative to the
 * ini), optionally nuisance_params (a .paramnames of five names; default
 * alpha_SZ ystar_SZ bias_SZ scatter_SZ beta_SZ) and the option keys of the
 * reference's run ini: 2D, prior_alpha_SZ, prior_ystar_SZ, prior_scatter_SZ,
 * prior_beta_SZ, prior_wtg, prior_lens, prior_cccp, prior_ns, prior_omegabh2.
 * 1D = T and any other key are CMBL_ERR_UNSUPPORTED, the key named in the
 * message; a ylims file whose row count is not patches x thetas, and fewer
 * than two thetas, are CMBL_ERR_FORMAT.  A walker's theory row is
 *     [H0, ns, ombh2, E[nzs], dA[nzs], grid[nzs][nm]]
 * (3 + 2 nzs + nzs nm doubles): E = H(z)/H0 and dA the angular diameter
 * distance in Mpc/h at steps_z, grid[j * nm + m] what get_grid leaves
 * (dndlnM deg2 dVdzdO, szcounts.f90:1317-1334) at steps_z[j] and mass
 * exp(31 + 0.05 (m + 1/2)) Msun/h.  The library uses the row as given; which
 * mass function filled it is the provider's business.  Nuisance parameters
 * in DataParams order (alpha, log10 ystar, bias, scatter, beta).
 * cmbl_sz_info: dims[8] = nzs, nm, redshift bins Nz, S/N bins, thetas,
 * patches, ln Y nodes, catalogue rows kept.  cmbl_sz_arrays: steps_z [nzs],
 * DNcat [Nz][S/N bins], and the 0-based steps j1[Nz], j2[Nz] between which a
 * redshift bin is integrated; any pointer may be NULL.  CMBL_ERR_ARG for
 * another likelihood. */
int  cmbl_sz_info(const cmbl_t *h, int *dims);
int  cmbl_sz_arrays(const cmbl_t *h, double *steps_z, double *dncat, int *j1, int *j2);

/* "MPK" (mpk.f90) and "WIGGLEZ" (wigglez.f90): the galaxy power-spectrum
 * likelihoods, bias and Q marginalised inside as the reference does; no
 * nuisance parameters, cl_lmax all zero.  A walker's theory row is
 *     [a_scl, kh_min, P[nk]]
 * (2 + nk doubles, nk the kbands used): a_scl = DV_fid / (H0 D_V(z)), exactly 1
 * without use_scaling (compute_scaling_factor, mpk.f90:46-56); kh_min =
 * exp(PK%x(1)), the lower edge of the provider's k grid; P[i] =
 * PowerAt(max(kh_min, a_scl k_i), z) as the provider's interpolator returns it,
 * before the division by a_scl^3 and the GiggleZ factor.  The library forms
 * k_scaled = max(kh_min, a_scl k_i) again from the row and does the rest of
 * MPK_LnLike (:312-407) / WiggleZ_LnLike (:545-641), single-precision normV, Q
 * and minchisq and the running normV of WiggleZ included.
 * "MPK" keys (MPK_ReadIni :117-244): name, num_mpk_points_full,
 * num_mpk_kbands_full, min/max_mpk_points_use, min/max_mpk_kbands_use,
 * kbands_file, measurements_file, windows_file, cov_file (its selected block is
 * inverted once on the host), use_scaling with DV_fid (missing:
 * CMBL_ERR_FORMAT), redshift (0.35), Q_marge, Q_flat, Q_mid, Q_sigma, Ag (1.4),
 * and the override key mpk_dataset_nonlinear, which only says which P(k) the
 * provider is to use.  "WIGGLEZ" keys (TWiggleZCommon_ReadIni and
 * WiggleZ_ReadIni :203-437): those, the seven Use_*-hr_region switches (none
 * set: CMBL_ERR_FORMAT), redshift (within 0.001 of 0.22, 0.41, 0.6 or 0.78),
 * Use_gigglez (without nonlinear_wigglez = T: CMBL_ERR_FORMAT),
 * nonlinear_wigglez, num_conflicts, type_conflict1, name_conflict1 (read, not
 * acted on), and gigglez_dir, the directory of
 * gigglezfiducialmodel_matterpower_{a..d}.dat (default: the dataset's; an
 * extension, the reference uses its global data directory).  Any other key,
 * name = twodf and name = lrg_2009 are CMBL_ERR_UNSUPPORTED; more than 64
 * points used is CMBL_ERR_UNSUPPORTED.
 * Where the reference stops the program the walker's -lnL is CMBL_LOGZERO, for
 * that walker alone: a row entry that is NaN or Inf, a_scl <= 0, a k_scaled
 * outside the GiggleZ spline's knots, a 2 x 2 matrix of the Q_flat branch that
 * is not positive definite, normV <= 0, and a value that is not finite.
 * cmbl_mpk_info: dims[8] = points used, kbands used, regions used, zbin (0 for
 * "MPK"), Q mode (0 Q_marge = F, 1 Q_flat, 2 the Gaussian Q grid, 3 Q_sigma =
 * 0), has_cov, use_scaling, use_gigglez.  cmbl_mpk_arrays: the selected k [nk],
 * the data vector [regions][np] and the inverse covariance [regions][np][np]
 * (without a cov_file the diagonal matrix of 1 / sdev^2); any pointer may be
 * NULL.  CMBL_ERR_ARG for another likelihood. */
int  cmbl_mpk_info(const cmbl_t *h, int *dims);
int  cmbl_mpk_arrays(const cmbl_t *h, double *k, double *data, double *invcov);

/* "JLA_MARGE": n_grid the (alpha, beta) grid points the likelihood integrates
 * over (those the reference keeps), n_points the grid's points, grid_bytes the
 * device memory of their inverse covariance matrices (0 with diag_errors).
 * Any pointer may be NULL.  CMBL_ERR_ARG for another likelihood. */
int  cmbl_jla_marge_info(const cmbl_t *h, int *n_grid, int *n_points, size_t *grid_bytes);

/* Derived parameters a likelihood outputs per sample (the '*' names of its
 * nuisance .paramnames): their count and space-separated names (pointer owned
 * by the handle).  0 for most datasets. */
int  cmbl_derived_info(const cmbl_t *h, int *n_derived, const char **derived_names);

/* The derived parameters at W points (device pointers, asynchronous on
 * `stream`): nuis [W] x n_nuis (stride ld_nuis) as for cmbl_loglike_batch,
 * derived [W] x n_derived (stride ld_derived >= n_derived).  SMICA: the TT
 * foreground D_l at l = 2000 (TSmica_planck_derivedParameters); other
 * datasets: zeros (TDataLikelihood_derivedParameters).  The reference's
 * functions read no theory, so none is passed. */
int  cmbl_derived_batch(cmbl_t *h, int W, const double *nuis, long long ld_nuis,
                        double *derived, long long ld_derived, void *stream);

/* Bytes of device workspace cmbl_loglike_batch needs for W walkers. */
size_t cmbl_workspace_size(const cmbl_t *h, int W);

/* -lnL for W walkers (device pointers, asynchronous on `stream`):
 *   dl    [W] x [10 fields] x [l]  (strides ld_walker, ld_field, 1);
 *         ld_walker = 0 gives every walker the same theory (one slow point)
 *   nuis  [W] x n_nuis (stride ld_nuis)   -- DataParams of each walker
 *   out   [W]
 * workspace: cmbl_workspace_size(h, W) bytes of device memory, or NULL to use
 * the handle's own (then calls on one handle must not overlap). */
int  cmbl_loglike_batch(cmbl_t *h, int W,
                        const double *dl, long long ld_field, long long ld_walker,
                        const double *nuis, long long ld_nuis,
                        double *out, void *workspace, void *stream);

/* The same launch over W walker slots of which only [0, *wcount) are live
 * (wcount a device int, read by the kernels): the sampler's per-likelihood
 * change mask evaluates a likelihood this way on the compacted walkers whose
 * parameters moved.  out of a slot at or beyond *wcount is not written.  A live
 * slot's result has the bits cmbl_loglike_batch gives the same inputs.
 * CMBL_ERR_UNSUPPORTED for a likelihood without the sparse form (exact
 * CMBlikes, SPTpol). */
int  cmbl_loglike_batch_sparse(cmbl_t *h, int W,
                               const double *dl, long long ld_field, long long ld_walker,
                               const double *nuis, long long ld_nuis,
                               double *out, void *workspace, void *stream, const int *wcount);

/* Same with HOST arrays: stages through pinned host memory and device buffers
 * the handle keeps between calls (no allocation per call once sized), runs on
 * the handle's own stream and synchronises.  For hosts that keep C_l in CPU
 * memory, e.g. the reference's LogLike called per evaluation with W = 1
 * (INTEGRATION.md).  Reads only the theory the likelihood uses: fields up to
 * the last with cl_lmax > 0, each to its lmax (cmbl_theory_len doubles of
 * field 0 for a likelihood that has one).  One host call at a time per
 * handle (serialised internally). */
int  cmbl_loglike_batch_host(cmbl_t *h, int W,
                             const double *dl, long long ld_field, long long ld_walker,
                             const double *nuis, long long ld_nuis, double *out);

/* clik-compatible entry (source/cliklike.f90:138-166): each walker row of
 * cl_and_pars (stride ld) holds C_l (not D_l) for l=0..lmax of TT, EE, BB,
 * TE, TB, EB (lmax per spectrum from clik_lmax[6], -1 = absent) followed by
 * the nuisance parameters.  Writes +lnL (= -(-lnL)) like clik_compute.
 * Device pointers. */
int  cmbl_clik_compute_batch(cmbl_t *h, int W, const int *clik_lmax,
                             const double *cl_and_pars, long long ld,
                             double *lnlike, void *workspace, void *stream);
/* Device workspace bytes cmbl_clik_compute_batch needs for W walkers
 * (workspace NULL: the handle's own, grown on demand; such calls are serialised
 * on the host and ordered on the device after the previous one, whatever its
 * stream; asynchronous either way). */
size_t cmbl_clik_workspace_size(const cmbl_t *h, int W);

/* Sticky numerical status of a handle, set on device by the likelihood
 * kernels (their -lnL output for the affected walker is NaN):
 *   CMBL_STATUS_HL_NOCONV  an HL eigensolve (CMBLikes_Transform, CMBlikes.f90:
 *                          861-914) did not converge in 40 Jacobi sweeps; the
 *                          reference's LAPACK call would stop the run
 *   CMBL_STATUS_PIPE_WAIT  a sampler's pipelined fast step (cmbs_step) gave up
 *                          waiting for its walkers' trial calibrations, so its
 *                          terms are not to be trusted (a safety net: the wait
 *                          ends by construction)
 * cmbl_status synchronises the device, writes the bits accumulated since the
 * last clear to *flags and clears them when clear != 0.  The host entry
 * (cmbl_loglike_batch_host) checks them itself and returns CMBL_ERR_NUMERIC. */
#define CMBL_STATUS_HL_NOCONV 1
#define CMBL_STATUS_PIPE_WAIT 2
int  cmbl_status(cmbl_t *h, int *flags, int clear);

/* Per-kernel device timing (HIP events around every library launch; off by
 * default).  cmbl_profile_read: accumulated milliseconds and launch count of
 * the kernel named `kernel` (e.g. "plik_quadform_pairs"); synchronises. */
void cmbl_profile_enable(int on);
void cmbl_profile_reset(void);
int  cmbl_profile_read(const char *kernel, double *total_ms, long long *count);

/* ------------------------------------------------------------------ */
/* Batched Metropolis sampler (W independent chains, one per walker).  */

typedef struct cmbs cmbs_t;

typedef struct {
    int n_walkers;
    int num_params;            /* length of P (all parameters, used or fixed) */
    int n_used;                /* number of varying parameters */
    const int *params_used;    /* n_used, 1-based indices into P (settings.f90:97) */
    int n_blocks;              /* BaseParams%param_blocks (slow -> fast) */
    const int *block_n;        /* n_blocks sizes */
    const int *block_params;   /* concatenated, 1-based indices into params_used */
    int slow_block_max;        /* blocks 1..slow_block_max are slow (propose.f90:151) */
    int oversample_fast;
    double propose_scale;      /* MCMC.f90:38 default 2.4 */
    double temperature;        /* calclike.f90 Temperature */
    const double *pmin, *pmax; /* num_params hard bounds */
    const double *prior_mean, *prior_std; /* num_params Gaussian priors, std 0 = none */
    int seed_ij, seed_kl;      /* RANMAR seeds of walker 0; walker w uses
                                  cmbs_walker_seed() (documented in DESIGN.md) */
    int first_walker;          /* global index of walker 0 (for sharding) */
    /* GetLogPriors (calclike.f90:111-134): a Gaussian prior on parameter i counts
     * when i is varying (in params_used) or include_fixed_parameter_priors is set
     * (BaseParameters.f90:170-181); linear-combination priors
     * ((dot(weights, P) - mean)/std)^2 over all num_params (:184-201), std 0 = none */
    int include_fixed_parameter_priors;
    int n_lincomb;
    const double *lincomb_weights;              /* n_lincomb x num_params, row-major */
    const double *lincomb_mean, *lincomb_std;   /* n_lincomb */
} cmbs_config_t;

/* walker w's RANMAR seeds (ij in 0..31328, kl in 0..30081) */
void cmbs_walker_seed(int seed_ij, int seed_kl, int walker, int *ij, int *kl);

int  cmbs_create(const cmbs_config_t *cfg, cmbs_t **out, char *errbuf, size_t errlen);
void cmbs_destroy(cmbs_t *s);
const char *cmbs_last_error(const cmbs_t *s);

/* proposal covariance of the used parameters, n_used x n_used row-major host
 * array (BlockedProposer_SetCovariance, propose.f90:210-244) */
int  cmbs_set_covariance(cmbs_t *s, const double *cov);

/* test_likelihood term (calclike.f90:180-199): -lnL += (P-c)^T C^-1 (P-c)/2
 * over params_used; cov is n_used x n_used (inverted here), center num_params. */
int  cmbs_set_test_gaussian(cmbs_t *s, const double *cov, const double *center);

/* Add a CMB likelihood evaluated on cached per-walker theory:
 * DataParams = P(nuisance_indices) (GeneralTypes.f90:642-646: the indices
 * AddNuisanceParameters assigns, :618-669, in any order and shared between
 * likelihoods, e.g. calPlanck for plik_lite and lensing), nuisance_indices
 * 1-based, n_nuis of them (cmbl_info).  dl is a device array laid out as for
 * cmbl_loglike_batch for this sampler's walkers; it must stay alive while the
 * sampler is used. */
int  cmbs_add_likelihood(cmbs_t *s, cmbl_t *like, const int *nuisance_indices,
                         const double *dl, long long ld_field, long long ld_walker);

/* Initial points (host, W x num_params) -> evaluates the starting -lnL. */
int  cmbs_set_start(cmbs_t *s, const double *P0, void *stream);

/* n_steps Metropolis steps for every walker.  fast_only != 0:
 * FastParameterSample (MCMC.f90:309-335, GetProposalFast) every step;
 * otherwise TMetropolisSampler_GetNewSample (MCMC.f90:269-307, GetProposal).
 * Asynchronous on stream.  The pipelined fast-step schedules hand data from
 * one workgroup to another inside a launch with bounded waits; a wait that
 * gives up marks the call's steps invalid, and the next cmbs_step or state /
 * history readback returns CMBL_ERR_NUMERIC ("... gave up waiting ..."). */
int  cmbs_step(cmbs_t *s, int n_steps, int fast_only, void *stream);

/* Fast dragging, TFastDraggingSampler_GetNewSample (MCMC.f90:338-452;
 * sampling_method = fast_dragging): n_steps GetNewSample calls for every
 * walker; every oversample_fast-th call drags the fast parameters (Neal) along
 * a slow proposal over interp_steps = max(2, nint(dragging_steps * num_fast) + 1)
 * interpolation steps (dragging_steps 3 by default, settings.f90:82), the
 * others are FastParameterSample.  Each drag needs the likelihoods at the
 * proposed slow point: `theory_fn` is called once per drag (synchronously,
 * after the slow proposal) with the device trial rows P_end [num_params][ld]
 * (walker-minor) and must fill every likelihood's end-theory buffer
 * registered with cmbs_set_trial_theory; it returns 0 on success.  Walkers
 * whose drag is accepted get their end theory copied into their theory rows
 * (the dl buffer passed to cmbs_add_likelihood).  With no likelihoods (the
 * analytic test target) theory_fn may be NULL.  Walkers whose CurLike is
 * logZero skip the drag (the reference makes a full Metropolis step there). */
typedef int (*cmbs_theory_fn)(void *user, int W, const double *P_end, long long ld, void *stream);
/* Trial-point theory buffer of likelihood `like_index` (same layout as its
 * theory rows), filled by the theory function for dragging end points and
 * for cmbs_step_theory trial points. */
int  cmbs_set_trial_theory(cmbs_t *s, int like_index, double *dl_end, long long ld_field, long long ld_walker);
int  cmbs_step_drag(cmbs_t *s, int n_steps, double dragging_steps, cmbs_theory_fn theory_fn, void *user,
                    void *stream);
/* Full TMetropolisSampler_GetNewSample steps (MCMC.f90:269-307; GetProposal
 * slow and fast) when data likelihoods need the theory at the trial point
 * (the reference recomputes it with CAMB, CalcLike_Cosmology.f90:59-94):
 * theory_fn fills the trial-theory buffers from the trial rows every step and
 * accepted walkers take the trial theory.  cmbs_step(fast_only = 0) refuses
 * slow proposals when data likelihoods are registered. */
int  cmbs_step_theory(cmbs_t *s, int n_steps, cmbs_theory_fn theory_fn, void *user, void *stream);

/* After cmbs_load_state of an image whose walkers moved their slow parameters
 * (cmbs_step_theory / cmbs_step_drag ran before the checkpoint), the walker
 * theory rows given to cmbs_add_likelihood hold whatever the new process put
 * there: every cmbs_step* call fails until this refreshes them.  theory_fn is
 * called once with the current points P [num_params][ld] and fills every
 * trial-theory buffer (cmbs_set_trial_theory), which is then copied into the
 * walkers' theory rows.  The reference likewise recomputes the theory at the
 * restart point (GeneralSetup.f90:123-131).  CurLike and the per-likelihood
 * terms stay as saved (not re-evaluated): theory_fn must reproduce the theory
 * the run had at those points. */
int  cmbs_refresh_theory(cmbs_t *s, cmbs_theory_fn theory_fn, void *user, void *stream);

/* ------------------------------------------------------------------ */
/* Polynomial theory calculator: the theory at a slow point from a response
 * surface of D_l, evaluated on the device (the place the reference gives its
 * calculator object; Calculator_PICO.f90 is its polynomial emulator, whose
 * error = 1 outside the training box becomes logZero, calclike.f90:308-313).
 *
 *   x_i      = (P[param_index_i] - center_i) / scale_i
 *   basis_k  = prod_i x_i^exponents[k][i]   (from 1.0, i ascending, every power
 *              by repeated multiplication)
 *   dl[w*ld_walker + fields[j]*ld_field + l] = sum_k basis_k(w) * coef[k][j][l],
 *              l = 0..lmax, fused multiply-adds in ascending k from +0.0;
 *              nothing else in the buffer is written
 * Walker w is valid iff every input has lo_i <= P_i <= hi_i (equality passes,
 * NaN fails: the sampler's own bound test, calclike.f90:97-109).  A walker
 * that is not is still evaluated, at its inputs clamped into the box (a NaN
 * first replaced by center_i), so the buffer never holds junk.  A walker's
 * result does not depend on W, on its place in the batch or on the strides. */
typedef struct cmbt cmbt_t;
typedef struct {
    int n_in;                 /* 1..16 input parameters */
    const int *param_index;   /* n_in, 1-based into P */
    const double *center, *scale;   /* x_i = (P_i - center_i) / scale_i, scale_i != 0 */
    const double *lo, *hi;    /* validity box on the raw P_i, lo_i <= hi_i */
    int n_terms;              /* 1..256 monomials */
    const int *exponents;     /* n_terms x n_in, row-major, each row's sum <= 4 (PICO's order) */
    int n_fields;             /* 1..CMBL_NFIELDS */
    const int *fields;        /* field indices 0..9 (TT=0 ... PP=9), no repeats */
    int lmax;
    const double *coef;       /* host, [n_terms][n_fields][lmax+1], l from 0 */
} cmbt_config_t;
/* Copies every table (the coefficients to the device); CMBL_ERR_ARG for a
 * count outside its range, an exponent row above order 4, a zero scale,
 * lo > hi, or a field index outside 0..9 or repeated. */
int  cmbt_create(const cmbt_config_t *cfg, cmbt_t **out, char *errbuf, size_t errlen);
void cmbt_destroy(cmbt_t *t);
const char *cmbt_last_error(const cmbt_t *t);
/* One launch, asynchronous on `stream`, for W points:
 *   P     device rows [num_params][ld], walker-minor: what cmbs_theory_fn receives
 *   dl    a theory buffer laid out as for cmbl_loglike_batch
 *   fail  device int[W], 1 for a walker outside the box, else 0; or NULL
 * CMBL_ERR_ARG for a param_index outside 1..num_params, ld < W,
 * ld_walker == 0 or ld_field < lmax + 1. */
int  cmbt_eval(cmbt_t *t, int W, const double *P, long long ld, int num_params,
               double *dl, long long ld_field, long long ld_walker, int *fail, void *stream);
/* Calculator-derived parameters: scalar response surfaces over the same
 * monomials, the parameterization's derived parameters of the reference's chain
 * rows (H0, omegam, sigma8, ..., DL40 .. DL2000: CosmologyParameterizations.f90:
 * 189-272, calclike.f90:447-448) and the hard cuts of TP_NonBaseParameterPriors
 * (CosmologyParameterizations.f90:90-112: logZero when H0 leaves [H0_min,
 * H0_max] or zre < use_min_zre, before any likelihood runs, calclike.f90:300-301).
 *
 *   out[d*ld_out + m] = sum_k basis_k(m) * coef[k][d],  d = 0..n_derived-1,
 * with the box test, clamp, monomials and fma chain of cmbt_eval: an output
 * whose coef column is a D_l coefficient column has cmbt_eval's bits of that
 * D_l, and a point's bits depend on neither M, its place nor the strides.
 * With lo or hi given the outputs are ranged: a point fails when any output
 * violates lo_d <= v <= hi_d (equality passes; a NaN value fails, also against
 * infinite limits).  With both NULL there is no range test. */
#define CMBT_MAXDERIVED 32
typedef struct {
    int n_derived;            /* 1..CMBT_MAXDERIVED */
    const double *coef;       /* host [n_terms][n_derived] */
    const double *lo, *hi;    /* n_derived each, or NULL = none; -inf / +inf = no limit on that side */
} cmbt_derived_config_t;
/* Copies the tables; replaces an earlier set; cfg == NULL removes it, and the
 * calculator is again exactly what cmbt_create made.  CMBL_ERR_ARG for
 * n_derived outside 1..32, a NULL coef, or lo > hi.  Not to be called while
 * work that uses the calculator is in flight. */
int  cmbt_set_derived(cmbt_t *t, const cmbt_derived_config_t *cfg);
int  cmbt_derived_count(const cmbt_t *t);
/* One launch (theory_derived_kernel), asynchronous on `stream`, for M points:
 *   P     device rows [num_params][ld], point-minor, as for cmbt_eval
 *   out   device [n_derived][ld_out], point-minor
 *   fail  device int[M]: 1 for a point outside the box (its outputs are those
 *         of the clamped inputs) or, when ranged, with an output outside its
 *         range; else 0; or NULL
 * CMBL_ERR_ARG with nothing set, for ld < M, ld_out < M or a param_index
 * outside 1..num_params.
 * Once ranges are set, cmbt_eval's own fail flags are box-or-range as well (a
 * second small launch in stream order; the D_l it writes keeps every bit), so
 * a sampler with this calculator rejects such trials as logZero and
 * cmbs_refresh_theory refuses such current points. */
int  cmbt_derived_eval(cmbt_t *t, int M, const double *P, long long ld, int num_params,
                       double *out, long long ld_out, int *fail, void *stream);
/* The calculator as the sampler's theory source: with theory_fn == NULL,
 * cmbs_step_theory and cmbs_step_drag evaluate it at the trial rows into every
 * distinct trial-theory buffer (cmbs_set_trial_theory), one launch each and
 * no host call or synchronisation inside the step loop, so all n_steps are
 * queued at once.  A trial outside the calculator's box has -lnL = logZero,
 * exactly as one outside the sampler's bounds (in a drag, such an end point
 * aborts the drag, MCMC.f90:370-374).  cmbs_refresh_theory evaluates it at
 * the current points and returns CMBL_ERR_NUMERIC, the walker theory rows
 * untouched, if any lies outside the box.  A non-NULL theory_fn still takes
 * precedence.  NULL removes the calculator.  Not owned: it must outlive the
 * sampler's use of it, and it is not part of the cmbs_save_state image (a
 * resumed run sets it again). */
int  cmbs_set_theory_calculator(cmbs_t *s, cmbt_t *calc);
/* A calculator of its own for likelihood like_index's trial-theory buffer
 * (e.g. JLA's distance moduli beside a D_l buffer): it fills that buffer in
 * place of the sampler's calculator, which still serves every other buffer and
 * the derived likelihoods.  A walker fails -- logZero in every term row -- when
 * any of the calculators flags it.  Likelihoods that share one trial buffer
 * share its calculator (the first override among them).  cmbs_refresh_theory
 * and the failure rule are as above; with no override set every launch is as
 * without this call.  NULL removes the override.  Not owned, and not part of
 * the cmbs_save_state image. */
int  cmbs_set_like_calculator(cmbs_t *s, int like_index, cmbt_t *calc);

/* ------------------------------------------------------------------ */
/* Gaussian likelihood on calculator-derived quantities: the reference's
 * Gaussian priors on derived parameters (H0_prior, zre_prior,
 * CosmologyParameterizations.f90:105-110) and its Gaussian background
 * likelihoods (TBAOLikelihood, bao.f90:265-308: D_V/r_s, D_M/r_s, H r_s, A(z),
 * f sigma8 at a dataset's redshifts), with the theory vector taken from n
 * scalar response surfaces over a calculator's monomials.
 *
 *   v_i    = sum_k basis_k(m) * coef[k][i]   box test, clamp, monomials and fma
 *            chain of cmbt_derived_eval: v_i has the bits cmbt_derived_eval
 *            gives for the same column
 *   r_i    = v_i - obs_i
 *   y_i    = fma(invcov[i][j], r_j, y_i), j ascending from +0.0
 *   s      = fma(r_i, y_i, s),            i ascending from +0.0
 *   out[m] = s / 2
 * A point outside the calculator's box (a NaN input included) has out[m] =
 * CMBL_LOGZERO exactly.  A point's bits depend on neither M, its place in the
 * batch nor ld. */
#define CMBG_MAXN 32
typedef struct cmbg cmbg_t;
typedef struct {
    int n;                    /* 1..CMBG_MAXN theory values */
    const double *coef;       /* host [n_terms][n]: n scalar surfaces over the calculator's monomials
                                 (what cmbt_set_derived takes) */
    const double *obs;        /* n */
    const double *invcov;     /* n x n row-major, symmetric bit for bit */
} cmbg_config_t;
/* Copies the tables: the object keeps coefficient columns of its own, apart
 * from what cmbt_set_derived holds.  `calc` is not owned and must outlive the
 * object.  CMBL_ERR_ARG for n outside 1..32, a NULL table, a non-finite obs or
 * invcov entry, or invcov[i][j] != invcov[j][i]. */
int  cmbg_create(cmbt_t *calc, const cmbg_config_t *cfg, cmbg_t **out, char *errbuf, size_t errlen);

/* Tabulated likelihoods on 1 or 2 such surfaces: the reference's BAO
 * likelihoods that are no Gaussians.  The object is a cmbg_t: cmbg_eval (one
 * launch of theory_table_kernel), cmbg_destroy, cmbg_last_error and
 * cmbs_add_derived_likelihood take it unchanged.  v_i is formed as above, so it
 * has cmbt_derived_eval's bits; every division below is an IEEE division, every
 * operation one rounding in the order written (no fma), as the reference
 * compiled without fast-math computes them.  r_drag enters the surfaces bare:
 * rs_rescale is not applied (get_rs_drag is called bare in both forms).
 *
 * CMBG_TABLE_1D (BAO_MGS_loglike, bao.f90:390-410), surface 0 = D_V / r_drag:
 *   alpha  = v_0 / scale                    scale = DVfid / rsfid, a double
 *   alpha > x_max or alpha < x_min:         out[m] = CMBL_LOGZERO
 *   ii     = floor((alpha - x_min) / step)  zero-based; step is the reference's
 *                                           default-real 0.001 as a double,
 *                                           (double)0.001f, not 0.001
 *   chi2   = (table[ii] + table[ii + 1]) / 2
 *   out[m] = chi2 / 2
 *
 * CMBG_TABLE_2D (BAO_DR1x_loglike, bao.f90:346-376), surface 0 = D_A / r_drag,
 * surface 1 = Hofz_Hunit * r_drag:
 *   a_perp = v_0 / DA_rd_fid
 *   a_plel = Hrd_fid / v_1                  v_1 = 0 gives +-inf: outside
 *   a_perp outside [perp[0], perp[np - 2]] or a_plel outside [plel[0],
 *   plel[np - 2]]:                          out[m] = CMBL_LOGZERO (the upper
 *                                           bound is the second-to-last knot)
 *   ii     = floor((a_perp - perp[0]) / (perp[1] - perp[0]))     zero-based,
 *   jj     = floor((a_plel - plel[0]) / (plel[1] - plel[0]))     no search
 *   prob   = (1 / ((perp[ii+1] - perp[ii]) * (plel[jj+1] - plel[jj]))) *
 *            (((prob[ii][jj]     * (perp[ii+1] - a_perp) * (plel[jj+1] - a_plel)
 *             - prob[ii+1][jj]   * (perp[ii]   - a_perp) * (plel[jj+1] - a_plel))
 *             - prob[ii][jj+1]   * (perp[ii+1] - a_perp) * (plel[jj]   - a_plel))
 *             + prob[ii+1][jj+1] * (perp[ii]   - a_perp) * (plel[jj]   - a_plel))
 *            each product left to right
 *   out[m] = prob > 0 ? -log(prob) : CMBL_LOGZERO
 *
 * Both: a NaN alpha compares false in the reference's bounds test; here it is
 * CMBL_LOGZERO.  A point outside the calculator's box (a NaN input included)
 * has out[m] = CMBL_LOGZERO and fail[m] = 1, as in cmbg_eval.  A point's bits
 * depend on neither M, its place in the batch nor ld. */
#define CMBG_TABLE_1D 1
#define CMBG_TABLE_2D 2
typedef struct {
    int form;                 /* CMBG_TABLE_1D or CMBG_TABLE_2D */
    const double *coef;       /* host [n_terms][1] (1-D) or [n_terms][2] (2-D): the surfaces */
    /* CMBG_TABLE_1D */
    int n;                    /* table entries, >= 2 */
    double scale, x_min, x_max, step;
    const double *table;      /* n */
    /* CMBG_TABLE_2D */
    int np;                   /* knots per axis (alpha_npoints), >= 3 */
    const double *perp;       /* np */
    const double *plel;       /* np */
    const double *prob;       /* [np][np], perp the outer index, already divided by its maximum */
    double DA_rd_fid, Hrd_fid;
} cmbg_table_config_t;
/* Copies the tables.  `calc` is not owned and must outlive the object.
 * CMBL_ERR_ARG for another form, a NULL table, a non-finite table entry, knot,
 * coefficient or parameter, scale or a fiducial 0, n < 2, np < 3, step <= 0,
 * x_min >= x_max, knot[1] - knot[0] <= 0 on either axis, and a table too short
 * for the cell the arithmetic above names at the upper bound: floor((x_max -
 * x_min) / step) + 1 >= n, or floor((knot[np - 2] - knot[0]) / (knot[1] -
 * knot[0])) + 1 >= np on either axis (computed on the host in the same
 * arithmetic; a point inside the bounds cannot get a larger index). */
int  cmbg_create_table(cmbt_t *calc, const cmbg_table_config_t *cfg, cmbg_t **out, char *errbuf, size_t errlen);
void cmbg_destroy(cmbg_t *g);
const char *cmbg_last_error(const cmbg_t *g);
/* One launch (theory_gauss_kernel), asynchronous on `stream`, for M points:
 *   P     device rows [num_params][ld], point-minor, as for cmbt_eval
 *   out   device [M]
 *   fail  device int[M]: 1 for a point outside the box, else 0; or NULL
 * Nothing outside out[0..M) and fail[0..M) is written.  CMBL_ERR_ARG for
 * ld < M or a param_index outside 1..num_params. */
int  cmbg_eval(cmbg_t *g, int M, const double *P, long long ld, int num_params,
               double *out, int *fail, void *stream);
/* The object as a likelihood of the sampler: one more term row after the data
 * likelihoods' (cur terms, history terms, the chi2_* chain columns, the
 * cmbs_save_state image, whose n_like counts both kinds), summed in
 * target_like after the data terms and divided by the temperature, where the
 * reference puts NonBaseParameterPriors and BAO (calclike.f90:300).  In call
 * order, at most 8 rows with the data likelihoods, whose cmbs_add_likelihood
 * calls all come first.  The rows are evaluated with cmbg_eval at the start
 * point and at the trial / drag-end rows of cmbs_step_theory and
 * cmbs_step_drag (also with a theory_fn: the derived rows still come from the
 * calculator); a fast step's trial keeps the walker's current term.  A
 * sampler with derived likelihoods alone steps with cmbs_step_theory /
 * cmbs_step_drag and needs no trial-theory buffer.  cmbs_set_theory_calculator
 * must be set to the calculator the objects were created on: otherwise
 * cmbs_set_start and the stepping entries return CMBL_ERR_ARG.  Not owned. */
int  cmbs_add_derived_likelihood(cmbs_t *s, cmbg_t *g);

/* Execution tuning (no reference counterpart; results are unchanged): split the
 * walkers into n_groups 64-aligned slices, each stepped on an internal stream
 * forked from / joined to the caller's, so the Metropolis kernel of one slice
 * overlaps the likelihood kernels of the others.  Default 1. */
int  cmbs_set_groups(cmbs_t *s, int n_groups);

/* Binned-theory cache (SURVEY 8(d)'s labelled variant, no reference
 * counterpart): inside one cmbs_step call of fast-only steps the theory is
 * fixed, and the window/bin sums of the theory are calibration-independent,
 * so with on != 0 the unified fast step bins each walker's theory once per
 * call and every step reuses those raw sums (the quadratic form, the small
 * chi^2 and the Metropolis chain still run every step, and the calibration is
 * applied to the sums as before, so the results are the same bits).  Only the
 * unified schedule (plik_lite + a small gaussian CMBlikes likelihood) uses it;
 * other runs ignore it.  Default 0: every step re-bins the theory, as the
 * reference's LogLike does. */
int  cmbs_set_binned_cache(cmbs_t *s, int on);

/* Optional history capture for convergence statistics: every step appends
 * each walker's current used-parameter vector and CurLike to a device ring of
 * `capacity` steps (SampleCollector AddNewPoint, SampleCollector.f90:324-456). */
int  cmbs_enable_history(cmbs_t *s, int capacity);
/* Per-walker statistics over history rows [first, last] (inclusive; row k is
 * the k-th step recorded since cmbs_enable_history, the ring keeps the last
 * `capacity`): means[W][n_used], covs[W][n_used][n_used], device ptrs
 * (SampleCollector.f90:235-246 "second half" window is first = count/2). */
int  cmbs_history_stats(cmbs_t *s, int first, int last, double *means, double *covs, void *stream);
int  cmbs_history_count(const cmbs_t *s);
/* Synchronising copy of history rows [first, first+count) (step indices as
 * cmbs_history_stats; the ring keeps the last `capacity`) to HOST memory: out[count][n_used + 1][W], per step the used parameters
 * then CurLike of every walker (the chain-file writer's input,
 * IO_OutputChainRow IO.f90:85-93). */
int  cmbs_history_host(cmbs_t *s, int first, int count, double *out);
/* This GPU's partial sums for the convergence / proposal-learning exchange
 * (TMpiChainCollector_UpdateCovAndCheckConverge, SampleCollector.f90:212-322):
 * each walker is one chain whose samples are history rows [first, last].
 * Device out:
 *   gmean == NULL: [sum count, sum count*mean (n), sum count*cov (n*n),
 *                   sum cov (n*n), number of chains]      (2 + n + 2n^2)
 *   gmean != NULL: sum count*(mean-gmean)(mean-gmean)^T    (n^2)
 * where n = n_used.  Summed over GPUs these give the reference's pooled
 * mean, MPICovMat, mean-of-covariances and covariance-of-means. */
int  cmbs_chain_moments(cmbs_t *s, int first, int last, const double *gmean, double *out, void *stream);

/* Sample collector (TMpiChainCollector_AddNewPoint, SampleCollector.f90:324-460):
 * every walker's Samples list -- the thinned points the convergence test
 * windows over -- kept on device as a ring of history step numbers (the points
 * stay in the history ring).  cmbs_collector_enable after cmbs_enable_history;
 * sample_capacity bounds each walker's list (Samples%Thin keeps it below
 * the reference's 500000).  Part of the cmbs_save_state image once enabled. */
int  cmbs_collector_enable(cmbs_t *s, int sample_capacity);
/* AddNewPoint for history steps steps[0..n_steps) (increasing; host array)
 * of every walker: sample_num++, keep every MPI_thin_fac-th, Samples%Add (points
 * at logZero are skipped, MCMC.f90:146); with check_burn, the burn-in test
 * (a used parameter changed > 51 times between consecutive samples once
 * Count > 51, :352-377) and on burn DeleteRange to the last min_sample_update
 * samples (:391-397).  Synchronises; fails if a list outgrows its capacity. */
int  cmbs_collector_add(cmbs_t *s, const int *steps, int n_steps, int min_sample_update, int check_burn,
                        void *stream);
/* HOST copies of every walker's list start/count, Burn_done and MPI_thin_fac (any may be NULL). */
int  cmbs_collector_state_host(cmbs_t *s, int *start, int *count, int *burn_done, int *thin_fac);
/* Samples%Thin(2) and MPI_thin_fac * 2 for every walker whose Count > limit (:300-304). */
int  cmbs_collector_thin(cmbs_t *s, int limit, void *stream);
/* As cmbs_chain_moments, each walker over its own window: items Count/2 .. Count
 * of its list, Count - Count/2 + 1 samples (:233-246), its weight in the sums. */
int  cmbs_collector_moments(cmbs_t *s, const double *gmean, double *out, void *stream);
/* CheckLimitsConverge's per-chain limits (:477-544): ConfidVal (samples.f90:70-110)
 * of used parameters params[0..n_check) (0-based) over each walker's window at
 * limfrac (MPI_Limit_Converge): out[W][n_check][2] = (lower, upper), device
 * pointer; synchronises. */
int  cmbs_collector_limits(cmbs_t *s, const int *params, int n_check, double limfrac, double *out, void *stream);

/* Device pointers of the walker state (valid until destroy), walker-minor:
 * P [num_params][W], cur_like [W], mult [W] (double), num_accept [W] (int). */
int  cmbs_state(cmbs_t *s, double **P, double **cur_like, double **mult, int **num_accept);

/* Synchronising copy of the walker state to HOST arrays (any may be NULL):
 * P [W][num_params], cur_like [W], mult [W], num_accept [W]. */
int  cmbs_get_state_host(cmbs_t *s, double *P, double *cur_like, double *mult, int *num_accept);

/* Checkpoint / resume (replaces TMpiChainCollector_SaveState / ReadState,
 * SampleCollector.f90:139-202, and TChainSampler_SaveState / LoadState,
 * MCMC.f90:199-218).  The image is every walker's complete chain state
 * (point, CurLike, multiplicity, accept count, RANMAR state, proposer
 * cycle/rotation state), so a resumed chain continues exactly where it
 * stopped; the reference restarts from the last chain row with a new random
 * sequence instead.  The proposal covariance is not in the image: restore it
 * with cmbs_set_covariance first.  Loading checks the sampler shape and marks
 * the sampler started (no cmbs_set_start needed). */
size_t cmbs_state_bytes(const cmbs_t *s);
int  cmbs_save_state(cmbs_t *s, void *host_buf, size_t bytes);
int  cmbs_load_state(cmbs_t *s, const void *host_buf, size_t bytes);

/* Each likelihood's -lnL at the recorded points, history rows [first,
 * first + count), to HOST memory: out[count][n_likelihoods][W] in
 * cmbs_add_likelihood order (TCalculationAtParamPoint%Likelihoods: the
 * chi2_<tag> = 2 x term derived columns of a chain row, GeneralTypes.f90:767-776). */
int  cmbs_history_terms_host(cmbs_t *s, int first, int count, double *out);

/* Put history rows [first, first + count) back (HOST arrays laid out as
 * cmbs_history_host / cmbs_history_terms_host write them, terms may be NULL;
 * count <= capacity) and continue the ring at first + count: the samples the
 * convergence exchange windows over survive a resume (Samples%LoadState,
 * SampleCollector.f90:167). */
int  cmbs_history_restore(cmbs_t *s, int first, int count, const double *rows, const double *terms);

#ifdef __cplusplus
}
#endif
#endif
