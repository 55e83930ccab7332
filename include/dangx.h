/*
 * dangx.h -- C ABI of libdangx.so, the MI355X (gfx950) implementation of dang's
 * Gibbs inner loop.  Plain pointers and sizes only; no C++/torch types.
 *
 * The reference (hermda02/dang, Fortran 90) has no FFI layer; the seam is its
 * module API.  Each entry point below names the reference procedure whose work it
 * replaces.  A Fortran driver binds these through ISO_C_BINDING
 * (fortran/dangx_mod.f90); INTEGRATION.md shows the reference-side wrapper.
 *
 * Array layouts are the Fortran arrays as they sit in memory (no transposition):
 *   sig_map/rms_map (0:npix-1, nmaps, nbands)  == C [band][map][pix]
 *   masks           (0:npix-1, nmaps)          == C [map][pix]   (plane 1 is tested,
 *                                                 as everywhere in the reference)
 *   c%amplitude     (0:npix-1, nmaps)          == C [map][pix]
 *   c%indices       (0:npix-1, nmaps, nind)    == C [ind][map][pix]
 * All reals are IEEE fp64 (real(dp)); map numbers are 1-based (1=T,2=Q,3=U).
 *
 * A context holds ONE pixel shard [pix0, pix0+npix) of the sky on ONE device.
 * Every per-pixel operation is shard-local; the random streams are keyed by the
 * GLOBAL pixel index, so results do not depend on how the sky is sharded.
 * Global reductions (chi^2) are returned as un-normalised local sums for the
 * caller to all-reduce.
 *
 * Return value: 0 on success, non-zero on error (message: dangx_last_error).
 * The reference's convention is print + stop (e.g. src/dang_cg_mod.f90:97-101);
 * the Fortran wrapper reproduces that from the status code.
 */
#ifndef DANGX_H
#define DANGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DANGX_MAX_BANDS 32
#define DANGX_MAX_COMPS 16
#define DANGX_MAX_IND 2
#define DANGX_MAX_GROUP 8

/* component type == c%type string, src/dang_component_mod.f90:791-809 */
/* DANGX_TCMB: 'T_cmb' -- evaluate_T_cmb (:815-848); its eval_signal is the bare sed (:770-771).  Supported by
 * dangx_eval_sed, wherever a component is REMOVED from the data / summed into the sky model, as an index-sampled
 * component (per pixel or full sky), and as an amplitude-sampled member of a CG group: there the reference treats it as
 * a diffuse member whose mixing element is eval_sed (src/dang_cg_mod.f90:469, 691, 807 test only for template / hi_fit /
 * monopole), i.e. it solves for a c%amplitude that eval_signal then ignores -- reproduced as it is. */
enum { DANGX_POWERLAW = 1, DANGX_MBB = 2, DANGX_FREEFREE = 3, DANGX_LOGNORMAL = 4, DANGX_CMB = 5, DANGX_TCMB = 6,
       /* global-amplitude types: one amplitude per fitted band instead of one per pixel (c%template,
        * c%template_amplitudes, c%corr, c%nfit; src/dang_component_mod.f90:536-710).  A CG group that contains
        * them is a coupled system: DANGX_SOLVER_CG runs the reference's iteration on the device, DANGX_SOLVER_DIRECT
        * eliminates the per-pixel blocks and solves the Schur system of the (<= 32) global rows exactly. */
       DANGX_TEMPLATE = 7, DANGX_MONOPOLE = 8, DANGX_HIFIT = 9 };
/* c%lnl_type / c%prior_type strings, src/dang_sample_mod.f90:383-400 */
enum { DANGX_LNL_CHISQ = 1, DANGX_LNL_MARGINAL = 2, DANGX_LNL_PRIOR = 3 };
enum { DANGX_PRIOR_GAUSSIAN = 1, DANGX_PRIOR_UNIFORM = 2, DANGX_PRIOR_JEFFREYS = 3 };
/* ml_mode string, src/dang_cg_mod.f90:254-267 */
enum { DANGX_ML_SAMPLE = 1, DANGX_ML_OPTIMIZE = 2 };
/* poltype bit flags, src/dang_util_mod.f90:228-292 */
enum { DANGX_FLAG_T = 1, DANGX_FLAG_Q = 2, DANGX_FLAG_U = 4, DANGX_FLAG_QU = 8 };
/* amplitude solver: DIRECT = per-(pixel,plane) Cholesky block solve (MI355X path);
 * CG = the reference's global conjugate-gradient iteration run on the device. */
enum { DANGX_SOLVER_DIRECT = 0, DANGX_SOLVER_CG = 1 };
/* fluctuation term: REFERENCE reproduces compute_sample_vector exactly, including
 * its two quirks (src/dang_cg_mod.f90:1008-1015 one eta for all bands; :1033-1040 no
 * component offset); CORRECT draws the textbook sum_nu T^t N^-1/2 eta_nu. */
enum { DANGX_FLUCT_CORRECT = 0, DANGX_FLUCT_REFERENCE = 1 };
/* what a chain at a coarser Nside (sample_nside < nside) reads of the swept component (dangx_set_coarse_model):
 * REFERENCE reproduces the reference -- c%amplitude(i,k), c%indices(i,..) and ddata%masks(i,1) of the FULL-resolution
 * arrays at the coarse pixel number i (src/dang_sample_mod.f90:362, 372-377, 548-563); DEGRADED reads the component's
 * amplitude planes and index maps degraded like the data (udgrade_ring) and skips where the degraded mask is masked. */
enum { DANGX_COARSE_REFERENCE = 0, DANGX_COARSE_DEGRADED = 1 };

/* kernel ids for dangx_profile_get / dangx_profile_get_planes */
enum {
    DANGX_K_AMP_DIRECT = 0, DANGX_K_INDEX_MH = 1, DANGX_K_SKY_CHISQ = 2, DANGX_K_REDUCE = 3,
    DANGX_K_CG_AX = 4, DANGX_K_CG_VEC = 5, DANGX_K_AMP_INDEX = 6, DANGX_K_MOMENTS = 7, DANGX_K_HIST = 8, DANGX_K_SIGNAL = 9,
    DANGX_K_CHAINS = 10,   /* the read-outs over several chains (dangx_chains_*): nothing else is ever counted here */
    DANGX_K_BATCH = 11,    /* the batched accumulators (dangx_moments_batches): one launch per accumulation, one more per merge */
    DANGX_K_ANGLE = 12,    /* the polarisation-angle accumulators (dangx_moments_angles): one launch per accumulation, two with an integrated band */
    DANGX_K_FIT = 13,      /* the goodness-of-fit accumulators (dangx_moments_fit): one launch per accumulation */
    DANGX_K_COUNT = 14
};

typedef struct dangx_ctx dangx_ctx;

typedef struct {
    int32_t npix;         /* pixels in this shard */
    int32_t nmaps;        /* 1 or 3 (global nmaps, src/dang.f90:49-63) */
    int32_t nbands;       /* global nbands */
    int32_t ncomp;        /* global ncomp */
    int64_t pix0;         /* global index of this shard's first pixel */
    int64_t npix_global;  /* 12*nside^2 */
    int32_t device;       /* HIP device ordinal, -1 = current device */
    int32_t reserved;
} dangx_dims;

/* mirrors the fields of type(dang_comps) the hot path reads, src/dang_component_mod.f90:12-48 */
typedef struct {
    int32_t type;              /* DANGX_POWERLAW ... */
    int32_t is_synch;          /* trim(c%label)=='synch' (jeffreys prior, src/dang_lnl_mod.f90:289) */
    int32_t nindices;
    int32_t cg_group;          /* c%cg_group (1-based as in the parameter file) */
    int32_t sample_amplitude;  /* c%sample_amplitude */
    int32_t reserved;
    double nu_ref;             /* Hz */
    int32_t lnl_type[DANGX_MAX_IND];
    int32_t prior_type[DANGX_MAX_IND];
    double gauss_prior[DANGX_MAX_IND][2]; /* mean, std */
    double uni_prior[DANGX_MAX_IND][2];   /* low, high */
    double step_size[DANGX_MAX_IND];
} dangx_comp_desc;

/* ---- lifetime ------------------------------------------------------------ */
int dangx_create(dangx_ctx **ctx, const dangx_dims *dims);
int dangx_destroy(dangx_ctx *ctx);
const char *dangx_last_error(const dangx_ctx *ctx);
const char *dangx_version(void);
/* run all work of this context on the given hipStream_t (NULL = default stream) */
int dangx_set_stream(dangx_ctx *ctx, void *hip_stream);
/* Pixel-sharded runs (one context per rank, dangx_dims.pix0/npix = the rank's RING range): the few places where the
 * reference sums over the WHOLE sky inside a call -- the dot products of cg_search (src/dang_cg_mod.f90:279-312) and
 * the global-amplitude rows of compute_rhs / compute_Ax / compute_sample_vector (:522-587, :833-893, :1045-1096) --
 * hand their local sums (host doubles, n <= 32*32+96; the coarse-Nside sweeps of a pixel shard: their degrade buffers) to this callback, which must replace buf[0..n) by its sum over
 * all ranks and return 0 (an MPI_Allreduce(MPI_IN_PLACE, buf, n, MPI_DOUBLE, MPI_SUM) or a torch.distributed
 * all_reduce).  is_root != 0 on exactly one rank: the replicated global rows are counted there in dot products.
 * fn == NULL (the default) = single rank.  Every rank must make the same sequence of calls. */
typedef int (*dangx_allreduce_fn)(void *user, double *buf, int64_t n);
int dangx_set_allreduce(dangx_ctx *ctx, dangx_allreduce_fn fn, void *user, int is_root);
int dangx_synchronize(dangx_ctx *ctx);
/* number of HIP devices visible to the process (a single-process driver creates one context per device) */
int dangx_device_count(int *n);
/* Host map arrays of the calls below (dangx_upload_data, dangx_put / get_amplitude / indices, dangx_set_template, the
 * sky / res / chi_map outputs of dangx_sky_model_chisq) are by default packed per shard, [planes][npix].  A driver
 * that keeps FULL-SKY arrays -- the reference's sig_map(0:npix-1,nmaps,nbands) etc. -- and runs several pixel-shard
 * contexts over them (one per GPU) passes, for each context, the address of the shard's FIRST pixel in plane 1 and sets
 * plane_stride = the full-sky pixel count here: plane q of the shard then starts plane_stride doubles after plane
 * q-1.  plane_stride = 0 returns to the packed layout. */
int dangx_set_host_stride(dangx_ctx *ctx, int64_t plane_stride);

/* ---- static description (once, after src/dang.f90:73) ------------------------ */
/* bp(j): src/dang_bp_mod.f90:7-15,31-57.  n = 0 for a 'delta' bandpass, else n
 * samples nu0[] (Hz) with normalised weights tau0[].  band is 0-based. */
int dangx_set_band(dangx_ctx *ctx, int band, double nu_c_hz, int n, const double *nu0, const double *tau0);
int dangx_set_component(dangx_ctx *ctx, int comp /*0-based*/, const dangx_comp_desc *desc);
/* global T_CMB used by the 'cmb' SED through a2t (src/dang_util_mod.f90:15) */
int dangx_set_tcmb(dangx_ctx *ctx, double T_cmb);
/* ddata%gain(:), ddata%offset(:) (src/dang_data_mod.f90:31-32) */
int dangx_set_calibration(dangx_ctx *ctx, const double *gain, const double *offset);

/* Unit conversions of a band (src/dang_bp_mod.f90): a2t [uK_cmb/uK_RJ] :211-243, a2f [MJy sr-1/uK_RJ] :181-209 (its
 * single-precision `1e14` literal included), f2t [uK_cmb/(MJy sr-1)] :245-274, evaluated on the host from the band set
 * with dangx_set_band (delta: at nu_c; otherwise the tau0-weighted sum over the samples) and the current T_CMB. */
enum { DANGX_A2T = 0, DANGX_A2F = 1, DANGX_F2T = 2 };
int dangx_unit_conversion(dangx_ctx *ctx, int band, int which, double *out);
/* normalize_bandpass, src/dang_bp_mod.f90:62-81: tau_out = tau_in / sum(tau_in) (what init_bp_mod applies to tau0
 * before the hot path sees it); no context needed */
int dangx_normalize_bandpass(const double *tau_in, int n, double *tau_out);
/* convert_maps, src/dang_data_mod.f90:429-463, on the RESIDENT maps: for every band with cg_map[j] == 0 (cg_map may be
 * NULL = none swapped) conversion[j] = 1 (uK_RJ), 1/a2t (uK_cmb) or 1/a2f (MJy/sr); sig_map(:,:,j), rms_map(:,:,j) and
 * offset(j) are multiplied by it and the offsets are copied into template_amplitudes(:,1) of every monopole.
 * conversion[nbands] is an output (ddata%conversion).  Call after dangx_upload_data / dangx_adopt_device_data (adopted
 * buffers are scaled in place). */
enum { DANGX_UNIT_UK_RJ = 0, DANGX_UNIT_UK_CMB = 1, DANGX_UNIT_MJY_SR = 2 };
int dangx_convert_maps(dangx_ctx *ctx, const int32_t *unit, const int32_t *cg_map, double *conversion);

/* ---- map data ------------------------------------------------------------------ */
/* ddata%sig_map, rms_map, masks: host pointers, copied to HBM */
int dangx_upload_data(dangx_ctx *ctx, const double *sig, const double *rms, const double *mask);
/* same arrays already resident in HBM (borrowed, not copied, not freed) */
int dangx_adopt_device_data(dangx_ctx *ctx, const double *sig_dev, const double *rms_dev, const double *mask_dev);
/* c%amplitude(:, :) and c%indices(:, :, :) of component comp; host pointers */
int dangx_put_amplitude(dangx_ctx *ctx, int comp, const double *amp);
int dangx_get_amplitude(dangx_ctx *ctx, int comp, double *amp);
int dangx_put_indices(dangx_ctx *ctx, int comp, const double *ind);
int dangx_get_indices(dangx_ctx *ctx, int comp, double *ind);
/* global-amplitude components: c%template ([map][pix], host pointer, copied), c%corr(j) (1 = band j is fitted),
 * c%nfit; and c%template_amplitudes(band, map) exchanged as [map][band] */
int dangx_set_template(dangx_ctx *ctx, int comp, const double *tmpl, const int32_t *corr, int nfit);
int dangx_put_template_amplitudes(dangx_ctx *ctx, int comp, const double *ta);
int dangx_get_template_amplitudes(dangx_ctx *ctx, int comp, double *ta);
/* let caller-owned HBM buffers BE the resident amplitude / index maps of a component
 * (borrowed, not freed; idx_dev may be NULL when the component has no indices) */
int dangx_adopt_device_state(dangx_ctx *ctx, int comp, double *amp_dev, double *idx_dev);
/* device addresses of the resident copies ([map][pix] and [ind][map][pix]) */
void *dangx_amplitude_devptr(dangx_ctx *ctx, int comp);
void *dangx_indices_devptr(dangx_ctx *ctx, int comp);

/* ---- amplitude phase: one (group, flag) pass of sample_cg_groups ---------------
 * replaces compute_rhs + cg_search + unpack_amplitudes (src/dang_cg_mod.f90:166-171).
 * flag is one poltype bit (T, Q, U or Q+U).  seed/stream select the keyed random
 * stream (the reference uses an unseeded RANDOM_NUMBER, src/dang.f90:67).
 * cg_iters (nullable): CG iteration counter as printed by the reference (CG solver); 0 for DIRECT, or -k when the
 * DIRECT solve of a group with template / monopole / hi_fit members found k directions of the global amplitudes
 * that the diffuse members absorb completely (those keep their current value, as they do under the reference's CG).
 * n_not_spd (nullable): units whose block was not SPD (left unchanged). */
int dangx_amp_sample(dangx_ctx *ctx, int group, int flag, int ml_mode, int solver, int fluct_mode,
                     uint64_t seed, uint64_t stream, int i_max, double converge,
                     int *cg_iters, int64_t *n_not_spd);

/* Accuracy of the last DANGX_SOLVER_DIRECT solve of a group with template / monopole / hi_fit members, measured
 * directly at the new state after the last step of iterative refinement (b, A: the system of compute_rhs /
 * compute_sample_vector / compute_Ax, src/dang_cg_mod.f90:326-1096): rel_residual[0] = the largest |b - A x| over the
 * global rows relative to that row of b; rel_residual[1] = the same relative to the size of the row's terms
 * (sum |b terms| + |A x terms|: rounding alone leaves ~1e-16 sqrt(npix) there, and weakly constrained amplitudes are
 * large, so [0] can sit well above [1]); refinements = steps taken (0: the first solution already met 1e-12).
 * A well-conditioned system of `template` members (every pivot of the equilibrated Schur matrix >= 1e-3) is not measured: both numbers are then the
 * a-priori bound 16 R eps / (smallest pivot) and refinements = 0; the environment variable DANGX_SCHUR_CHECK=1 measures always. */
int dangx_schur_info(dangx_ctx *ctx, double *rel_residual /*[2]*/, int *refinements);
/* Residual of the reference's linear system at the CURRENT amplitudes, through the reference's own operators
 * (dangx_compute_rhs + dangx_compute_sample_vector(eta(seed, stream)) - dangx_compute_Ax(x), vectors kept on the device):
 * out[0] = |b - A x|_2 / |b|_2 over the rows of unmasked units and the global rows, out[1] = the largest global-row
 * residual relative to that row of b (0 without global members).  What cg_search's delta_new measures
 * (src/dang_cg_mod.f90:285, 303); call it with the seed / stream / ml_mode of the solve it checks. */
int dangx_amp_residual(dangx_ctx *ctx, int group, int flag, int ml_mode, uint64_t seed, uint64_t stream, double *out);

/* ---- index phase: sample_index_mh, per-pixel branch (src/dang_sample_mod.f90:88-485,
 * index_mode==2, sample_nside==nside).  nind 0-based; map_n = 1,2,3 or -1 (Q+U).
 * accepted (nullable): number of accepted proposals over the shard. */
int dangx_index_sample(dangx_ctx *ctx, int comp, int nind, int map_n, int nsample, int ml_mode,
                       uint64_t seed, uint64_t stream, int64_t *accepted);

/* ---- two consecutive indices of ONE component on the same planes, in one call: exactly
 * dangx_index_sample(comp, nind, map_n, nsample, ml_mode, seed, stream_first, accepted_first) followed by
 * dangx_index_sample(comp, nind + 1, map_n, nsample, ml_mode, seed, stream_second, accepted_second) -- consecutive passes of
 * the loop over a component's indices in sample_spectral_parameters (src/dang_sample_mod.f90:40-75; dust beta, then dust T)
 * -- and bit for bit their result.  Nothing the second sweep removes from the data has changed in between, so where the
 * register chain covers both indices they run in ONE launch on one staging of the maps. */
int dangx_index_sample_pair(dangx_ctx *ctx, int comp, int nind, int map_n, int nsample, int ml_mode, uint64_t seed,
                            uint64_t stream_first, uint64_t stream_second, int64_t *accepted_first, int64_t *accepted_second);

/* ---- the amplitude solve of a CG group and the FIRST index sweep on the same planes, in one call: exactly
 * dangx_amp_sample(group, flag, ml_mode, solver, fluct_mode, seed_amp, stream_amp, i_max, converge, cg_iters, n_not_spd) followed by
 * dangx_index_sample(comp, nind, map_n, nsample, ml_mode, seed_index, stream_index, accepted) -- the way sample_cg_groups
 * (src/dang_cg_mod.f90:142-177) and sample_spectral_parameters (src/dang_sample_mod.f90:21-86) follow each other plane set by
 * plane set in the main loop (src/dang.f90) -- and bit for bit their result.  When every step is independent per pixel
 * (delta bands, diffuse members only, direct solver, reference fluctuation term, chisq likelihood with a gaussian / uniform
 * prior, the sampled component a member of the group whose other members are the only other components on these planes)
 * both run in ONE kernel launch: the maps are read once and the solve's arithmetic hides under the chain's. */
int dangx_amp_index_sample(dangx_ctx *ctx, int group, int flag, int ml_mode, int solver, int fluct_mode, uint64_t seed_amp,
                           uint64_t stream_amp, int i_max, double converge, int comp, int nind, int map_n, int nsample,
                           uint64_t seed_index, uint64_t stream_index, int *cg_iters, int64_t *n_not_spd, int64_t *accepted);

/* ---- everything one iteration does on ONE plane set of a CG group, in one call: exactly
 * dangx_amp_sample(group, flag, ml_mode, solver, fluct_mode, seed_amp, stream_amp, i_max, converge, cg_iters, n_not_spd) followed by
 * dangx_index_sample(comp[s], nind[s], map_n(flag), nsample, ml_mode, seed_index, stream[s], &accepted[s]) for s = 0 .. nsweeps-1 --
 * the solve of sample_cg_groups (src/dang_cg_mod.f90:166-171) and the passes of sample_spectral_parameters on these planes
 * (src/dang_sample_mod.f90:40-75) in the reference's order (the caller passes them in that order; dangx_plan_fusion says when the
 * grouping leaves the main loop's result unchanged).  For models with many bands and members whose swept components are all
 * members of the group (C5) this is ONE kernel launch that keeps the members' SED columns in LDS across the sweeps instead of
 * evaluating every other member's SED again in every sweep; every other case IS the calls above (through dangx_amp_index_sample
 * and dangx_index_sample_pair where they apply).  accepted[nsweeps] nullable. */
int dangx_plane_set_sample(dangx_ctx *ctx, int group, int flag, int ml_mode, int solver, int fluct_mode, uint64_t seed_amp,
                           uint64_t stream_amp, int i_max, double converge, int nsweeps, const int32_t *comp, const int32_t *nind,
                           const uint64_t *stream, int nsample, uint64_t seed_index, int *cg_iters, int64_t *n_not_spd,
                           int64_t *accepted);

/* ---- the index phase of ONE plane set in one call: exactly
 * dangx_index_sample(comp[s], nind[s], map_n(flag), nsample, ml_mode, seed, stream[s], &accepted[s]) for s = 0 .. nsweeps-1 -- the
 * passes of sample_spectral_parameters (src/dang_sample_mod.f90:40-75) that touch the planes of `flag`, in the reference's order:
 * what the two-call seam (src/dang.f90:101, 106) issues after sample_cg_groups has returned.  Sweeps on disjoint planes are
 * independent (c%indices(:, k, :) is per plane), so a caller may collect the sweeps of a plane set from the reference's
 * component-major loop.  Where every swept component is an amplitude-sampled member of ONE CG group whose members are the only
 * components on these planes (delta bands, chisq likelihood, gaussian / uniform priors) the sweeps are ONE kernel launch on the
 * amplitudes in memory: one staging of the maps, the residual kept in registers between the sweeps; every other case IS the
 * calls above (consecutive indices of a component through dangx_index_sample_pair).  accepted[nsweeps] nullable. */
int dangx_plane_sweeps_sample(dangx_ctx *ctx, int flag, int nsweeps, const int32_t *comp, const int32_t *nind, const uint64_t *stream,
                              int nsample, int ml_mode, uint64_t seed, int64_t *accepted);

/* ---- sky model + chi^2: update_sky_model + compute_chisq
 * (src/dang_data_mod.f90:339-396, 494-526).  pol_lo..pol_hi = ddata%pol_type range.
 * chisq_sum receives the LOCAL sum over unmasked pixels and planes of
 * sum_j res^2/rms^2 (not divided by nbands or nump); the reference's chisq is
 * allreduce(chisq_sum)/nbands/nump.  sky/res ([band][map][pix]) and chi_map
 * ([map][pix], already divided by nbands as in the reference) are optional host outputs. */
int dangx_sky_model_chisq(dangx_ctx *ctx, int pol_lo, int pol_hi, double *chisq_sum,
                          double *sky, double *res, double *chi_map);
/* asynchronous form: writes the local sum to a device double (for an RCCL all-reduce) */
int dangx_sky_model_chisq_dev(dangx_ctx *ctx, int pol_lo, int pol_hi, double *chisq_sum_dev);

/* chi^2 sums that the index sweeps compute as a by-product (no extra pass over the maps):
 * which = 0: the state the amplitude phase left (captured by the first sweep on each plane since its last
 * amplitude update), which = 1: the current state.  Same un-normalised local sum as above.  Returns 2 when
 * a plane in pol_lo..pol_hi was not covered by a sweep -- fall back to dangx_sky_model_chisq. */
int dangx_chisq_cached(dangx_ctx *ctx, int which, int pol_lo, int pol_hi, double *chisq_sum);
int dangx_chisq_cached_dev(dangx_ctx *ctx, int which, int pol_lo, int pol_hi, double *chisq_sum_dev);

/* the same number for the CURRENT state at the least cost: cached sums where the last sweeps left them, one explicit pass over
 * each remaining plane (whose sum is then cached too).  What gpu_chisq of the reference-side wrapper calls after every CG group
 * and every phase (write_stats_to_term, src/dang_data_mod.f90:528-570). */
int dangx_chisq_current(dangx_ctx *ctx, int pol_lo, int pol_hi, double *chisq_sum);

/* ---- index phase with sample_nside /= nside (src/dang_sample_mod.f90:199-217, 332-483) --------------------------
 * One whole-sky context (npix = 12*nside^2, pix0 = 0), or a pixel shard with an all-reduce (see below).  As in the reference: the data minus every other component is
 * formed at full resolution, then degraded with HEALPix's udgrade_ring (RING -> NEST, mean of the good children,
 * NEST -> RING), the rms with dang's udgrade_rms (sqrt(mean(rms^2)) * nside_out/nside_in), the mask with udgrade_mask
 * (mean >= 0.5); one chain per COARSE pixel i; the coarse index map is upgraded (children take the parent's value) and
 * written to c%indices(:, s1:s2, nind) for EVERY pixel.  Also as in the reference, the chain of coarse pixel i reads
 * the FULL-resolution arrays at the same index i (ddata%masks(i,1), c%indices(i,...), and eval_signal's
 * c%amplitude(i,k): src/dang_sample_mod.f90:362, 372-377, 548-553): reproduced literally, see DESIGN.md section 7 -- unless
 * dangx_set_coarse_model chose DANGX_COARSE_DEGRADED for (comp, nind), below.
 * HEALPix itself is absent from the reference tree (an external library): udgrade_ring / nest2ring are restated from
 * the published algorithm (Gorski et al. 2005, ApJ 622, 759; HEALPix 3.x pix_tools / udgrade_nr).
 * Likelihoods: chisq / marginal / prior; priors: gaussian / uniform / jeffreys; diffuse component types and T_cmb. */
int dangx_index_sample_coarse(dangx_ctx *ctx, int comp, int nind, int map_n, int nsample, int ml_mode,
                              uint64_t seed, uint64_t stream, int nside, int sample_nside, int64_t *accepted);
/* On a PIXEL SHARD (pix0 /= 0 or npix /= 12*nside^2) dangx_index_sample_coarse needs sums over all shards -- the
 * children of a coarse pixel are scattered over the RING ranges -- and takes them through the dangx_set_allreduce callback
 * (one process per GPU; the buffers below, i.e. up to 2*(2*Sp*nbands+1)*12*sample_nside^2 doubles, not the few of the
 * amplitude solves).  A single process that drives several contexts calls the three phases itself and ADDS the buffers
 * of all contexts between them, in shard order:
 *   dangx_coarse_sizes     : lengths of the two buffers (n_partials; n_index = 12*sample_nside^2 + 1)
 *   dangx_coarse_partials  : A -- per coarse pixel and plane the sum of this shard's good children and their number, for the
 *                            cleaned data, rms^2 and the mask -> buf[n_partials]
 *   dangx_coarse_chains    : B -- finish data / rms / mask from the SUMMED partials; run the chains of the coarse pixels i
 *                            whose full-resolution pixel i this shard holds -> index_out[0..npc) (0 elsewhere),
 *                            index_out[npc] = accepted proposals
 *   dangx_coarse_writeback : C -- c%indices(:, s1:s2, nind) of this shard's pixels from the SUMMED coarse index map
 * With one shard the result equals the whole-sky call bit for bit; with several the child sums are associated
 * differently (each shard's children first), i.e. the degraded maps agree to rounding. */
int dangx_coarse_sizes(dangx_ctx *ctx, int map_n, int sample_nside, int64_t *n_partials, int64_t *n_index);
int dangx_coarse_partials(dangx_ctx *ctx, int comp, int map_n, int nside, int sample_nside, double *buf);
int dangx_coarse_chains(dangx_ctx *ctx, int comp, int nind, int map_n, int nsample, int ml_mode, uint64_t seed, uint64_t stream,
                        int nside, int sample_nside, const double *partials_sum, double *index_out);
int dangx_coarse_writeback(dangx_ctx *ctx, int comp, int nind, int map_n, int nside, int sample_nside, const double *index_sum);
/* The coarse model of index nind (0-based) of component comp: DANGX_COARSE_REFERENCE (the default) or DANGX_COARSE_DEGRADED.
 * Sticky per context; set it on EVERY context of a sky.  With DEGRADED the chain of coarse pixel p reads
 *   amp_c[k](p) = udgrade_ring(c%amplitude(:,k)), k = s1..s2 (mean of the children in NESTED order, dangx_udgrade mode 0),
 *   idx_c[n](p) = udgrade_ring(c%indices(:,s1,n)) for every index n (the swept one is the chain's start, the others enter the SED),
 * and is skipped where the degraded mask is masked -- a skipped pixel keeps its starting value idx_c (the reference's 0 is
 * no usable index: a dust temperature of 0 makes the children's SEDs NaN); data / rms / mask, likelihoods, priors, bounds,
 * draw slots and the write-back (children take the parent's value) are unchanged.  The full-sky chain at a coarser Nside and
 * its tuner use amp_c.  Honoured by dangx_index_sample_coarse (whole sky, and shards through dangx_set_allreduce),
 * dangx_fullsky_sample, dangx_tune_step_size and the dangx_sky_* wrappers.
 * Several contexts of one process drive DEGRADED with three more entries between phases A and B (the three-phase entries
 * above keep their buffers and results):
 *   dangx_coarse_model_size     : length of the model buffer, (Sp + nindices + 1) * 12*sample_nside^2 -- 0 when no index of
 *                                 comp runs DEGRADED (then there is nothing to add, and the two calls below refuse)
 *   dangx_coarse_model_partials : per coarse pixel this shard's child sums of the Sp amplitude planes and nindices index
 *                                 maps, then the number of those children (one count: amplitudes are never MISSVAL)
 *   dangx_coarse_model_finish   : the degraded amplitudes / indices from the SUMMED buffer, valid until the state changes;
 *                                 also before dangx_tune_step_size on shards prepared by dangx_fullsky_finish_coarse
 * dangx_coarse_chains (and dangx_tune_step_size) of a DEGRADED index without finished model sums for the current state fail. */
int dangx_set_coarse_model(dangx_ctx *ctx, int comp, int nind, int model);
int dangx_coarse_model_size(dangx_ctx *ctx, int comp, int map_n, int sample_nside, int64_t *n_model);
int dangx_coarse_model_partials(dangx_ctx *ctx, int comp, int map_n, int nside, int sample_nside, double *buf);
int dangx_coarse_model_finish(dangx_ctx *ctx, int comp, int map_n, int nside, int sample_nside, const double *model_sum);
/* the degrade / upgrade primitives on their own (whole-sky context): mode 0 = udgrade_ring, 1 = udgrade_rms,
 * 2 = udgrade_mask(threshold 0.5); host pointers, one map each ([12*nside_in^2] -> [12*nside_out^2]) */
int dangx_udgrade(dangx_ctx *ctx, int mode, const double *map_in, int nside_in, double *map_out, int nside_out);

/* ---- per-iteration trace output without pulling maps: mask_avg(c%indices(:,map_n,nind), masks) as printed by
 * write_data every Gibbs iteration (src/dang_data_mod.f90:716-731, src/dang_util_mod.f90:186-206).  Returns this
 * shard's sum over unmasked pixels and their number; mask_avg = (all-reduced sum) / (all-reduced count). */
int dangx_index_masked_sum(dangx_ctx *ctx, int comp, int nind, int map_n, double *sum, int64_t *count);

/* n <= 16 such sums in one launch and one wait: (comp[e], nind[e], map_n[e]) -> sums[e], counts[e] */
int dangx_index_masked_sums(dangx_ctx *ctx, int n, const int32_t *comp, const int32_t *nind, const int32_t *map_n, double *sums,
                            int64_t *counts);

/* Step-size tuning in the per-pixel branch (src/dang_sample_mod.f90:341-346) starts the tuner's sky-wide chain at
 * sample(l) = sum(c%indices(:,map_inds(1),l)) / sum(mask(:,1)): both sums run over EVERY pixel and the mask VALUES are
 * summed.  Returns this shard's two sums; the chain itself is dangx_fullsky_prepare / dangx_fullsky_sums (below). */
int dangx_index_plain_sum(dangx_ctx *ctx, int comp, int nind, int map_n, double *sum_index, double *sum_mask);

/* ---- full-sky index mode (index_mode == 1, src/dang_sample_mod.f90:229-329), tune_spectral_parameter_length
 * (:623-717) and fit_band_gain (:570-621).  With one index for the whole sky every Metropolis step is one pass
 * that yields a few global sums; the chain (proposal, prior, accept, step-size tuning) stays with the caller,
 * between its all-reduces (dang_amd/api.py: sample_index_mh_fullsky, tune_spectral_parameter_length,
 * fit_band_gain).
 *   dangx_fullsky_prepare: data_raw minus every other component for the planes of map_n (:173-196), kept in HBM.
 *   dangx_fullsky_sums   : LOCAL sums at theta[2]: what = 0 evaluate_lnL (1 value); 1 evaluate_marginal_lnL
 *                          (2*nbands*Sp values: TNd(j,k), TNT(j,k) interleaved, j outer / k inner; the caller forms
 *                          sum -1/2 TNd^2/TNT after the all-reduce); 2 the jeffreys-prior sum (1 value).
 *                          3 the chisq likelihood's sufficient statistics about theta (3*nbands*Sp values: W0, U, V of
 *                          (band j, plane k) at 3*(j*Sp + k): sum r0^2, sum r0 a/sigma, sum a^2/sigma^2 with r0 = (d - a s_j(theta))/sigma).
 *   dangx_fill_index     : c%indices(:, s1:s2, nind) = value for every pixel (:329, :483).
 *   dangx_gain_sums      : out[0] = sum map2*N_inv*map1, out[1] = sum map1*N_inv*map1 of fit_band_gain (:606-607). */
int dangx_fullsky_prepare(dangx_ctx *ctx, int comp, int map_n);
/* the same mode with c%sample_nside(nind) /= nside (:199-217): the cleaned data, the rms and the mask are degraded first
 * (udgrade_ring / udgrade_rms / udgrade_mask), dangx_fullsky_sums then runs over the 12*sample_nside^2 coarse pixels --
 * with eval_signal's c%amplitude read from the full-resolution array at the coarse pixel number, as in the reference
 * (see dangx_index_sample_coarse; with DANGX_COARSE_DEGRADED for any index of comp the degraded amplitude is made too, and
 * dangx_fullsky_sample / dangx_tune_step_size read it for those indices).  One whole-sky context. */
int dangx_fullsky_prepare_coarse(dangx_ctx *ctx, int comp, int map_n, int nside, int sample_nside);
int dangx_fullsky_sums(dangx_ctx *ctx, int what, const double *theta, double *out, int nout);
int dangx_fill_index(dangx_ctx *ctx, int comp, int nind, int map_n, double value);
int dangx_gain_sums(dangx_ctx *ctx, int band, double *out);
/* c%indices(pix, map_n, :) of one local pixel (the full-sky chain starts from pixel 0, :240-242) */
int dangx_peek_indices(dangx_ctx *ctx, int comp, int map_n, long long pix, double *out);

/* dangx_fullsky_prepare_coarse for a PIXEL SHARD: dangx_coarse_partials of every shard (map_n's planes), the buffers
 * added over the shards, then this call on every shard with the sum.  The degraded data / rms / mask are then whole-sky
 * on each shard, and dangx_fullsky_sums adds, per shard, the coarse pixels i whose full-resolution pixel i it holds
 * (that is where the reference reads c%amplitude(i), src/dang_sample_mod.f90:548-563).  dangx_fullsky_sample does this. */
int dangx_fullsky_finish_coarse(dangx_ctx *ctx, int comp, int map_n, int nside, int sample_nside, const double *partials_sum);

/* ---- the SKY-WIDE steps of the Gibbs loop, chain included (dang_amd/csrc/dangx_sky.hip) --------------------------------
 * One number describes the whole sky in these steps: a Metropolis step is a pass over the maps that leaves a few sums, plus
 * a few scalar operations -- or, for the chisq likelihood of a diffuse component (whose model of a band is amplitude(pixel) x
 * one SED value), ONE pass per sweep that leaves the sufficient statistics W0, U, V per (band, plane) about the starting point:
 * -2 lnL(theta) = sum [W0 - 2 ds U + ds^2 V], every proposal then costs nbands SED evaluations on the host (dangx_fullsky_sums
 * selector 3; the same chain to rounding, DANGX_FULLSKY_STATS=0 for a pass per proposal).  Each entry point runs the whole chain of the reference procedure it names, so the chain exists
 * once for every host language.  ctxs[0..nctx) are the contexts of THIS process in shard order (nctx = 1: a whole-sky
 * context, or one context per process); a sky-wide sum is the contexts' sums added in shard order, then summed over the
 * ranks through ctxs[0]'s dangx_set_allreduce callback.  Random numbers: Philox4x32-10 keyed by (seed, stream, pixel label
 * 2^40 - 1, running draw counter) -- the same on every rank.  Errors: dangx_last_error(ctxs[0]).
 *
 * dangx_fullsky_sample: sample_index_mh with index_mode == 1 (src/dang_sample_mod.f90:229-329) for index nind (0-based) of
 *   component comp on map_n (1, 2, 3 or -1 = Q+U): data_raw minus the other components (:173-196; degraded when
 *   sample_nside /= nside, :199-217; 0 or nside = full resolution), start at c%indices(0, map_inds(1), :) (:240-242), the
 *   tuner when tuned[nind] == 0 (:272-275), nsample steps (:282-324), c%indices(:, s1:s2, nind) = result (:329, :483).
 *   tuned[nindices] in/out = c%tuned (NULL: all tuned); step_size out (nullable) = c%step_size(nind) after the call (the
 *   contexts' descriptors are updated); value out (nullable) = the sampled index; accepted out (nullable).
 * dangx_tune_step_size: tune_spectral_parameter_length (:623-717) on data prepared by dangx_fullsky_prepare[_coarse] on every
 *   context; theta_init[2]; *draw = running draw counter of the stream (in/out).  +-50 % until the acceptance over nsample
 *   steps is within [0.4, 0.6]; then c%tuned = .true. for ALL indices (:712).  Bounded at 64 rounds (the reference's
 *   `do while (.not. c%tuned(nind))` does not return when nothing is accepted any more).
 * dangx_tune_perpixel: the 'Tuning!' block of the per-pixel branch (:337-346): one tuner pass per index l of the component,
 *   starting at sample(l) = sum(c%indices(:,map_inds(1),l)) / sum(mask(:,1)) over EVERY pixel (mask VALUES summed).
 * dangx_fit_band_gain: fit_band_gain(ddata, 1, band) (:570-621), band 0-based: gain = mu (optimize) or mu + sigma*N(0,1)
 *   (draw slot = band); stored as ddata%gain(band) on every context (:619) and returned.
 * dangx_update_tcmb: "Update the global variable T_CMB" (:75-78): T_CMB = c%indices(0,1,1) of a 'T_cmb' component, set on
 *   every context (it enters a2t of the 'cmb' SED) and returned. */
int dangx_fullsky_sample(dangx_ctx *const *ctxs, int nctx, int comp, int nind, int map_n, int nsample, int ml_mode,
                         uint64_t seed, uint64_t stream, int nside, int sample_nside, int32_t *tuned, double *step_size,
                         double *value, int64_t *accepted);
int dangx_tune_step_size(dangx_ctx *const *ctxs, int nctx, int comp, int nind, int nsample, int ml_mode, uint64_t seed,
                         uint64_t stream, const double *theta_init, uint32_t *draw, int32_t *tuned, double *step_size);
int dangx_tune_perpixel(dangx_ctx *const *ctxs, int nctx, int comp, int nind, int map_n, int nsample, int ml_mode,
                        uint64_t seed, uint64_t stream, int32_t *tuned, double *step_size);
int dangx_fit_band_gain(dangx_ctx *const *ctxs, int nctx, int band, int ml_mode, uint64_t seed, uint64_t stream, double *gain);
int dangx_update_tcmb(dangx_ctx *const *ctxs, int nctx, int comp, double *tcmb);

/* ---- which solves may be issued together with the first index sweep on their planes (dangx_amp_index_sample) without changing
 * the result of the main loop (src/dang.f90:101-106 runs every solve of sample_cg_groups before any sweep of
 * sample_spectral_parameters).  pairs: the (group, flag) passes of the sampled CG groups in sample_cg_groups' order; sweeps: the
 * (component, index, flag) sweeps in sample_spectral_parameters' order (component-major), sweep_plain = 1 for an ordinary
 * per-pixel sweep at the map resolution with a tuned step.  first_sweep[npairs] out: position in the sweep list of the sweep
 * to issue with that solve, or -1.  Pure host logic on the context's descriptors; the rule is stated at its definition
 * (dang_amd/csrc/dangx_sky.hip). */
int dangx_plan_fusion(dangx_ctx *ctx, int npairs, const int32_t *pair_group, const int32_t *pair_flag, int nsweeps,
                      const int32_t *sweep_comp, const int32_t *sweep_nind, const int32_t *sweep_flag, const int32_t *sweep_plain,
                      int solver, int32_t *first_sweep);

/* ---- one (group, flag) pass of sample_cg_groups over SEVERAL contexts of one process (src/dang_cg_mod.f90:166-171).
 * Diffuse groups: dangx_amp_sample on every context (enqueued on all before the first result is awaited).  Groups with
 * template / monopole / hi_fit members couple all pixels through their global rows (:522-587, :833-893): with
 * DANGX_SOLVER_DIRECT every context eliminates its per-pixel blocks (pass 1), the Schur rows are added over the contexts
 * (shard order) and the ranks, the small system is solved once, every context back-substitutes (pass 2); the residual
 * check and the refinement steps are shared the same way.  nctx = 1 IS dangx_amp_sample.  DANGX_SOLVER_CG needs nctx = 1. */
int dangx_sky_amp_sample(dangx_ctx *const *ctxs, int nctx, int group, int flag, int ml_mode, int solver, int fluct_mode,
                         uint64_t seed, uint64_t stream, int i_max, double converge, int *cg_iters, int64_t *n_not_spd);

/* ---- dangx_plane_set_sample over SEVERAL contexts of one process: dangx_sky_amp_sample(ctxs, nctx, group, flag, ...) followed by
 * dangx_plane_sweeps_sample(ctxs[r], flag, nsweeps, comp, nind, stream, ...) on every context -- what sample_cg_groups
 * (src/dang_cg_mod.f90:166-171) and the passes of sample_spectral_parameters on the group's planes (src/dang_sample_mod.f90:40-75)
 * do for one (group, flag) pair.  Diffuse groups: dangx_plane_set_sample on every context.  Groups with global-amplitude members
 * (:522-587, :833-893) share their Schur rows over the contexts and ranks as in dangx_sky_amp_sample; when the global members are
 * `template` components, the plane-set kernel covers the model and the small system is well conditioned (every pivot of the
 * equilibrated Schur matrix >= 1e-3, which bounds the global rows' residual by ~1e-12 |b| without measuring it), the
 * back-substitution runs inside the launch that does the sweeps: per context pass 1 and ONE launch.  nctx = 1 IS
 * dangx_plane_set_sample.  accepted[nsweeps], n_not_spd, cg_iters (= -nullity for a coupled group) nullable. */
int dangx_sky_plane_set_sample(dangx_ctx *const *ctxs, int nctx, int group, int flag, int ml_mode, int solver, int fluct_mode,
                               uint64_t seed_amp, uint64_t stream_amp, int i_max, double converge, int nsweeps, const int32_t *comp,
                               const int32_t *nind, const uint64_t *stream, int nsample, uint64_t seed_index, int *cg_iters,
                               int64_t *n_not_spd, int64_t *accepted);

/* ---- secondary seams (type-bound procedures of dang_cg_group), host vectors in the
 * reference's packing [c1: plane1(npix), plane2(npix) | c2: ... ] -------------------- */
int64_t dangx_group_size(dangx_ctx *ctx, int group, int flag);
int dangx_compute_rhs(dangx_ctx *ctx, int group, int flag, double *b);                       /* :326 */
int dangx_compute_Ax(dangx_ctx *ctx, int group, int flag, const double *x, double *res);     /* :598 */
int dangx_compute_sample_vector(dangx_ctx *ctx, int group, int flag, const double *eta, double *res); /* :913 */
/* eval_sed(band, pix, map_n) for all local pixels of one component/band/map -> out[npix] (:778) */
int dangx_eval_sed(dangx_ctx *ctx, int comp, int band, int map_n, double *out);

/* ---- kernels specialised at run time (dang_amd/csrc/dangx_rtc.hip) -------------------------------------------------------
 * The register-resident Metropolis kernels and the fused solve + first sweep are templates on the band count, the plane
 * count and the group size; the library carries instantiations for 3 / 5 / 6 / 8 / 10 / 20 bands.  Any other model shape is
 * compiled by hiprtc from the library's own (embedded) headers on the first sweep that needs it and cached on disk
 * ($DANGX_CACHE_DIR, default ~/.cache/dangx); DANGX_RTC=0 disables this (such shapes then take the LDS-column kernels).
 *   dangx_rtc_kernels: how many kernels this context obtained that way, and (names nullable) their template-ids, one per line.
 *   dangx_rtc_compile: compile-only check (no device needed), e.g. ("dx_kern_chain.h", "dxk::k_index_mh_reg<1, 1, 9, 1>");
 *                      0 on success; log receives the compiler's messages (or the kernel's symbol). */
int dangx_rtc_kernels(dangx_ctx *ctx, int *n, char *names, int names_len);
int dangx_rtc_compile(const char *header, const char *name_expr, char *log, int log_len);

/* ---- posterior moments: write_maps every iteration (src/dang.f90:119-121) + scripts/make_mean_maps.py (return_mean_map,
 * return_std_map = np.std) on the device ----------------------------------------------------------------------------------
 * Running means and second moments of the chain state, accumulated in HBM (f64 Welford update, k_moments_accum) so that no map
 * leaves the device until the summaries are read once at the end.  Accumulation only READS the state: no chi^2 cache entry,
 * kept coarse slot or index sum is dropped, and the chain's results do not change.
 * sel[comp] (NULL = every plane of every component): bits 0-2 = amplitude planes T,Q,U (for template / monopole / hi_fit
 * members: rows [map] of c%template_amplitudes); bits 3+3j .. 5+3j = planes T,Q,U of index j (j < DANGX_MAX_IND).  A bit for a
 * plane or index the component does not have is an error.  Allocates the accumulators (two f64 planes per selected plane) and
 * sets the count to 0; calling it again starts over. */
int dangx_moments_begin(dangx_ctx *ctx, const int32_t *sel);
/* one sample of the current state -- the resident planes as dangx_get_amplitude / _get_indices would read them after all
 * issued work, caller-owned buffers of dangx_adopt_device_state included (resolved here, not at begin) -- enqueued on the
 * context's stream like the sampler's launches: no host wait (except once after a component's buffers were adopted again).
 * Not capturable in a hipGraph: the new count's 1/n is a by-value kernel argument.  Fails when dangx_set_component changed a
 * selected component's type or nindices since begin.  dangx_put_amplitude / _put_indices between calls are state: the next
 * accumulation takes what they wrote. */
int dangx_moments_accumulate(dangx_ctx *ctx);
int dangx_moments_count(dangx_ctx *ctx, int64_t *n);
/* what: 0 = amplitude, 1 + j = index j;  stat: 0 = mean, 1 = standard deviation sqrt(m2 / (n - ddof)) (ddof 0 = np.std).
 * out: host array laid out as dangx_get_amplitude / _get_indices (one index) lay it out ([map][pix], host stride honoured);
 * planes that are not selected are left untouched.  Errors (nothing written): n = 0, stat = 1 with n - ddof <= 0, comp or what
 * out of range, nothing selected for (comp, what), a template / monopole / hi_fit amplitude (read by _get_template). */
int dangx_moments_get(dangx_ctx *ctx, int comp, int what, int stat, int ddof, double *out);
/* the same into a device array [map][pix] of this shard (packed), asynchronously on the context's stream */
int dangx_moments_get_dev(dangx_ctx *ctx, int comp, int what, int stat, int ddof, double *out_dev);
/* template / monopole / hi_fit members: the moments of c%template_amplitudes, [map][band] as dangx_get_template_amplitudes */
int dangx_moments_get_template(dangx_ctx *ctx, int comp, int stat, int ddof, double *ta);
/* Second-order summaries of the same samples x_1..x_n (mean and m2 = sum (x_t - mean)^2 as above), streamed like the moments:
 *   lag-1 autocorrelation rho1 = [sum_{t=2..n} (x_t - mean)(x_{t-1} - mean)] / m2 (the biased acf estimator) and the AR(1)
 *   effective sample size ESS = n (1 - rho)/(1 + rho), rho = max(rho1, 0), of every selected plane when lag1 != 0 (rows of
 *   c%template_amplitudes included);
 *   cross terms C = sum (a_t - mean_a)(b_t - mean_b) of npairs pairs of selected pixel planes at the same pixel:
 *   pairs[p] = {comp_a, what_a, plane_a, comp_b, what_b, plane_b}, what as in dangx_moments_get, plane 0-based.
 * Legal after dangx_moments_begin and before the first dangx_moments_accumulate (count 0); a second call replaces the first,
 * dangx_moments_begin drops everything.  Errors (nothing changes, an earlier registration stays): count > 0, a plane that is not
 * selected, a template / monopole / hi_fit amplitude in a pair, a == b, npairs > DANGX_MAX_PAIRS, a failed allocation (one f64
 * plane per pair, three per plane when lag1 != 0).  With pairs an accumulation is two launches (the cross terms read the means
 * of the previous accumulation, so they go first), otherwise one. */
#define DANGX_MAX_PAIRS 64
int dangx_moments_pairs(dangx_ctx *ctx, int lag1, int npairs, const int32_t *pairs);
/* dangx_moments_get / _get_dev / _get_template additionally take stat 2 = rho1 and 3 = ESS (ddof ignored; an error when lag-1
 * is not tracked).  A sample that never moved (a masked pixel) and n = 1 give NaN: 0/0, as np.corrcoef does.
 * stat: 0 = covariance C / (n - ddof), 1 = correlation C / sqrt(m2_a m2_b) (NaN where either variance is 0); out: [npix] of this
 * shard.  Errors: pair out of range, n = 0, covariance with n - ddof <= 0. */
int dangx_moments_get_pair(dangx_ctx *ctx, int pair, int stat, int ddof, double *out);
/* the same into a device array, asynchronously on the context's stream */
int dangx_moments_get_pair_dev(dangx_ctx *ctx, int pair, int stat, int ddof, double *out_dev);
/* Per-pixel histograms of selected pixel planes, accumulated on the same samples as the moments (k_moments_hist, a launch of its own
 * per accumulation, only when something is registered), and their read-out as quantile / mode / count maps (k_hist_stat): what
 * scripts/parameter_plotter.py takes from a pixel's trace (np.percentile, corner's histograms) without a sample leaving the device.
 * Definitions (dang_amd/csrc/dx_hist_host.h; the kernels and the host evaluate the same inline functions):
 *   registration r = a pixel plane planes[r] = {comp, what, plane} (what as in dangx_moments_get, plane 0-based) with a range
 *     lo < hi (both finite), nbins in {8, 16, 32, 64} and counters of bits in {16, 32}, nbins * bits / 8 <= 128: a pixel's record is
 *     a power-of-two number of bytes <= 128 and never crosses a 128-byte memory request.
 *   bin of a sample x: counted iff x >= lo && x <= hi (NaN, +-inf are not); scale = nbins / (hi - lo) formed once in f64;
 *     b = min((int)((x - lo) * scale), nbins - 1) -- np.histogram(x, nbins, (lo, hi)) on generic data; on interior edges THIS is
 *     the definition.  N = sum of a pixel's counters; samples outside the range = dangx_moments_count - N.
 *   quantile q in (0, 1): target = q * (double)N; walking the bins in order with cum = the sum before bin b, the first bin with
 *     c_b > 0 && cum + c_b >= target gives lo + ((hi - lo) / nbins) * (b + (target - cum) / c_b); N = 0 gives NaN.  The value lies
 *     in the closed bin that holds the ceil(q N)-th smallest counted sample.
 *   mode: the centre of the fullest bin, the lowest on ties; N = 0 gives NaN.
 *   per-pixel range: a registration declared with range[r] = {-inf, +inf} takes two f64 maps lo[p], hi[p] over this shard's pixels
 *     (dangx_moments_hist_range_maps; the library copies them and owns the copy).  Pixel p is ON when lo[p] and hi[p] are finite,
 *     hi[p] > lo[p], and neither hi[p] - lo[p] nor nbins / (hi[p] - lo[p]) overflows; for an on pixel every rule above holds with
 *     that pixel's bounds, scale_p = (double)nbins / (hi[p] - lo[p]) being one IEEE division.  An off pixel counts nothing: its
 *     N = 0, its quantile and mode are NaN.  Handing in masked pixels as NaN is the normal case, not an error.  The checksum of a
 *     pair of maps -- FNV-1a (64 bit) over the little-endian words of lo[0..npix) then hi[0..npix) -- is part of the registration
 *     wherever registrations are compared (the HEAD fingerprint below, the read-outs over several chains).
 *   source: planes[r] = {comp, what, plane} reads a plane of the chain's state; planes[r] = {sig, DANGX_HIST_SIGNAL, 0} reads
 *     registered signal sig of the current dangx_moments_signals list (any kind, P included): the sample is the value
 *     k_moments_signal feeds to its Welford update, bit for bit, binned by that kernel itself behind the update (its HIST form takes
 *     the place of the plain one in the same launches; no histogram reads a signal: the plain form runs, as before).  A signal has
 *     no default range: it needs a global one or maps.  Further errors of dangx_moments_hist: a signal source while no signals are
 *     registered, sig out of range, the same signal twice, a signal without any range.  dangx_moments_signals refuses, by name, to
 *     replace the signal list while a histogram reads a signal: drop the histograms first (nreg = 0).
 * dangx_moments_hist: range[r] = {lo, hi}; range == NULL or a NaN lo = the default, which an index plane has (that index's uni_prior
 *   in the descriptor at registration time: the chain never leaves it, src/dang_sample_mod.f90:415) and an amplitude plane has not.
 *   Legal after dangx_moments_begin and before the first dangx_moments_accumulate, independent of dangx_moments_pairs (either order,
 *   neither drops the other); a second call replaces the first (nreg = 0: none), dangx_moments_begin drops it.  Errors (nothing
 *   changes, an earlier registration stays): count > 0, a plane that is not selected, a template / monopole / hi_fit amplitude
 *   (not a pixel plane), a bad nbins or bits or a record over 128 bytes, hi <= lo or a non-finite bound, an amplitude plane
 *   without a range, nreg > DANGX_MAX_HIST, the same plane twice, a failed allocation (nbins * bits / 8 bytes per pixel and
 *   registration).  With histograms registered dangx_moments_accumulate fails before touching anything, naming the limit, when the
 *   new count would exceed 2^bits - 1: no counter ever wraps or saturates.  range[r] = {-inf, +inf} declares a per-pixel range
 *   (any other non-finite bound stays an error); dangx_moments_accumulate then fails before touching anything, naming the
 *   registration, until its maps were handed in.
 * dangx_moments_hist_range_maps: lo, hi = host arrays [npix] of this shard for registration reg; legal after dangx_moments_hist and
 *   before the first dangx_moments_accumulate, only for a registration declared with {-inf, +inf}; a second call replaces the
 *   first.  dangx_moments_hist_range_get returns the maps; for a global-range registration it fills them with its constants.
 *   k_moments_hist takes the global-range registrations as before; the per-pixel ones go into one launch of a second form of
 *   it that streams lo and hi beside x (16 bytes more per pixel and sample, 16 * npix bytes of maps per registration).
 * dangx_moments_hist_get: the raw records [npix][nbins] of this shard as uint16_t (bits 16) or uint32_t (bits 32).
 * dangx_moments_hist_stat: stat 0 = the nq quantiles q[0..nq) as out[nq][npix] (1 <= nq <= 16, every q strictly inside (0, 1));
 *   stat 1 = the mode, stat 2 = N as f64 (out[npix]; nq and q ignored).  Errors: reg out of range, no sample accumulated, a bad stat.
 * The _dev forms write a device array of this shard, asynchronously on the context's stream. */
#define DANGX_MAX_HIST 32
#define DANGX_HIST_SIGNAL (-1)
int dangx_moments_hist(dangx_ctx *ctx, int nreg, const int32_t *planes, const double *range, int nbins, int bits);
int dangx_moments_hist_get(dangx_ctx *ctx, int reg, void *counts);
int dangx_moments_hist_get_dev(dangx_ctx *ctx, int reg, void *counts_dev);
int dangx_moments_hist_stat(dangx_ctx *ctx, int reg, int stat, int nq, const double *q, double *out);
int dangx_moments_hist_stat_dev(dangx_ctx *ctx, int reg, int stat, int nq, const double *q, double *out_dev);
int dangx_moments_hist_range_maps(dangx_ctx *ctx, int reg, const double *lo, const double *hi);
int dangx_moments_hist_range_maps_dev(dangx_ctx *ctx, int reg, const double *lo_dev, const double *hi_dev);
int dangx_moments_hist_range_get(dangx_ctx *ctx, int reg, double *lo, double *hi);
int dangx_moments_hist_range_get_dev(dangx_ctx *ctx, int reg, double *lo_dev, double *hi_dev);
/* Moments of component signals at a band, accumulated on the same samples (k_moments_signal: a launch of its own per accumulation, and a second one for the signals at bandpass-integrated bands,
 * only when something is registered): what write_maps' output_fg maps hold (c%eval_signal(band, pix, map),
 * src/dang_data_mod.f90:596-617) and scripts/make_mean_maps.py averages -- nonlinear in the sampled amplitude and indices, so
 * not derivable from their moments.  Definitions (dang_amd/csrc/dx_signal_host.h):
 *   spec[s] = {comp, band, kind}; kind 0, 1, 2 = plane T, Q, U, kind 3 = the polarised intensity P (nmaps == 3).
 *   one sample of kinds 0-2 at a pixel: amplitude * sed, ROUNDED as a product, sed as dangx_eval_sed(comp, band, kind + 1) returns
 *     it (delta and integrated bandpasses, spatially constant index planes, band units); the bare sed for T_cmb.  A NaN sample
 *     stays NaN; nothing is skipped (an all-zero amplitude plane gives 0 * sed).
 *   kind 3: sqrt(sQ * sQ + sU * sU) of those two rounded samples (two rounded products, a rounded sum).
 *   The update is k_moments_accum's on accumulators of the library's own (two f64 planes per signal).
 * dangx_moments_signals: legal after dangx_moments_begin and before the first dangx_moments_accumulate, independent of
 *   dangx_moments_pairs / _hist (either order, none drops another) and of the selection words (a signal's planes need not be
 *   selected; an empty selection plus signals is a valid run); a second call replaces the first (nsig = 0: none),
 *   dangx_moments_begin / _end drop it.  Errors (nothing changes, an earlier registration stays): count > 0, comp / band / kind
 *   out of range, a kind the model's nmaps does not have, a template / monopole / hi_fit member (its signal is a host-side
 *   amplitude, read by dangx_moments_get_template, times a fixed map), the same signal twice, nsig > DANGX_MAX_SIGNALS, a failed
 *   allocation.  dangx_moments_accumulate fails when a registered component changed type or nindices since.
 * dangx_moments_get_signal: stat 0 = mean, 1 = standard deviation sqrt(m2 / (n - ddof)); out: [npix] of this shard.  Errors: sig
 *   out of range, n = 0, a bad stat, stat = 1 with n - ddof <= 0.  The _dev form writes a device array, asynchronously on the
 *   context's stream.
 * Histograms of signals: dangx_moments_hist with a signal source (above).  The polarisation angle of a signal is a circular
 * statistic with accumulators of its own: dangx_moments_angles (below).  Not covered: lag-1 / pairs of signals, frequencies
 * that are not bands of the model. */
#define DANGX_MAX_SIGNALS 64
int dangx_moments_signals(dangx_ctx *ctx, int nsig, const int32_t *spec);
int dangx_moments_get_signal(dangx_ctx *ctx, int sig, int stat, int ddof, double *out);
int dangx_moments_get_signal_dev(dangx_ctx *ctx, int sig, int stat, int ddof, double *out_dev);
/* Posterior polarisation angle psi = atan2(U, Q) / 2 of a component's signal at a band, as a CIRCULAR statistic: the arithmetic
 * mean of psi samples is wrong wherever the posterior straddles +-pi/2 (two samples at +85 and -85 degrees average to 0, not to
 * 90).  Accumulated on the same samples by k_moments_angle, a launch of its own behind the signals' (a second one for the angles
 * at bandpass-integrated bands), only when something is registered.  Definitions (dang_amd/csrc/dx_angle_host.h):
 *   spec[a] = {comp, band}.  Per sample and pixel sQ, sU are exactly the rounded samples of signal kinds 1 and 2 of that
 *     (comp, band), P = sqrt(sQ * sQ + sU * sU) as kind 3 forms it, c = sQ / P = cos 2 psi, s = sU / P = sin 2 psi (two IEEE
 *     divisions).  P == 0 gives NaN and NaN stays: nothing is skipped.  No sign convention is applied: the angle is that of the
 *     Q, U maps as the model holds them.
 *   accumulators: two f64 planes per angle, Cbar and Sbar, the running means m = fma(x - m, 1/n, m) of c and s.
 *   stat 0  circular mean  0.5 * atan2(Sbar, Cbar), in [-pi/2, pi/2]
 *   stat 1  circular standard deviation of psi in radians  0.5 * sqrt(-2 * log(Rbar)); +inf where Rbar == 0; exactly 0 where
 *           Rbar >= 1 - 5 * 2^-53, the rounding of a unit vector's length (a chain that never moved reads 0, not 7.45e-9)
 *   stat 2  mean resultant length Rbar = min(1, sqrt(Cbar^2 + Sbar^2)); the clamp makes the std of a chain that never moved 0
 *   stat 3, 4  Cbar, Sbar as they are.  NaN propagates through every stat.
 * dangx_moments_angles: legal after dangx_moments_begin and before the first dangx_moments_accumulate, independent of
 *   dangx_moments_pairs / _hist / _signals / _batches and of the selection words; a second call replaces the first (nang = 0:
 *   none), dangx_moments_begin / _end drop it, dangx_moments_begin_like copies it into the holder.  Errors (nothing changes):
 *   count > 0, nmaps != 3, comp / band out of range, an unset component, a template / monopole / hi_fit member, a T_cmb
 *   component (its signal is a bare SED and has no direction), the same angle twice, nang > DANGX_MAX_ANGLES, a failed allocation.
 * dangx_moments_get_angle: out [npix] of this shard.  Errors: ang out of range, n = 0, a bad stat (5 needs several chains).
 * dangx_chains_get_angle (rules of dangx_chains_* below): pooled Cbar = sum_k (n_k / N) Cbar_k in list order, Sbar likewise
 *   (unequal counts allowed); stats 0-4 on the pooled pair; stat 5 = BETWEEN, the circular std of the chains' mean directions:
 *   u_k = (Cbar_k, Sbar_k) / sqrt(Cbar_k^2 + Sbar_k^2), (Cb, Sb) = (sum_k u_k) / K in list order, R_b = min(1, sqrt(Cb^2 +
 *   Sb^2)), result 0.5 * sqrt(-2 log R_b): what to set beside stat 1 to see chains sitting at different angles.  There is no
 *   circular R-hat: none is standard.
 * The section of an angle is family 7 ANGLE (below).  The _dev forms write device arrays asynchronously.
 * Not covered: histograms, quantiles and batches of an angle, a circular R-hat, debiasing of P, signals at frequencies that are
 * not bands of the model. */
#define DANGX_MAX_ANGLES 64
int dangx_moments_angles(dangx_ctx *ctx, int nang, const int32_t *spec);
int dangx_moments_get_angle(dangx_ctx *ctx, int ang, int stat, double *out);
int dangx_moments_get_angle_dev(dangx_ctx *ctx, int ang, int stat, double *out_dev);
/* Goodness-of-fit maps, accumulated on the same samples: the residual at a (band, plane) and the chi^2 map of a plane -- what
 * write_maps writes as <band>_residual_k*.fits and chisq_k*.fits (src/dang_data_mod.f90:619-634, 656-662) and
 * scripts/make_mean_maps.py averages into <band>_residual_mean.fits and chisq_mean.fits.  chi^2 is quadratic in all sampled
 * parameters at once, so neither it nor the std of a residual follows from any other accumulator.  k_moments_fit is ONE launch
 * per accumulation behind the others (DANGX_K_FIT), only when something is registered; no copy of the residual exists in memory.
 * Definitions (dang_amd/csrc/dx_fit_host.h):
 *   spec[i] = {what, band, plane}, plane 0, 1, 2 = T, Q, U; what 0 = the residual at `band`, what 1 = the chi^2 map (band = -1).
 *   one sample at a pixel, in update_sky_model + compute_chisq's expressions as dangx_sky_model_chisq evaluates them:
 *     x_c(j) = the ROUNDED product amplitude * sed of a diffuse member, template_amplitudes * sed of a template / hi_fit member,
 *     the bare sed of T_cmb (a monopole lives in the band offset); sky_j = their sum in component order from 0.0;
 *     r_j = (sig - offset_j) / gain_j - sky_j on T, sig - sky_j on Q, U, at EVERY pixel, masked ones included;
 *     chi^2 = (sum_j (r_j r_j) / (rms_j rms_j)) / nbands over ALL bands in band order, whichever residuals are registered, at
 *     unmasked pixels only (plane T's mask): at a masked pixel nothing is accumulated and mean and std read 0, as the
 *     reference's chi_map.  NaN / inf propagate; nothing else is skipped (no amp == 0 shortcut).
 *   Units are the model's (uK_RJ): the division by conversion(j) that write_maps applies to a residual stays with the caller.
 *   The update is k_moments_accum's on two f64 planes per item of the library's own: 16 B * npix per item (everything at the C3
 *   workload: 33 items = 6.6 GB; at C5: 63 items = 50 GB -- register what is looked at).
 * dangx_moments_fit: legal after dangx_moments_begin and before the first dangx_moments_accumulate, independent of every other
 *   registration and of the selection words; a second call replaces the first (nfit = 0: none), dangx_moments_begin / _end drop
 *   it, dangx_moments_begin_like copies it into the holder.  Errors (nothing changes, the item is named): count > 0, what / band /
 *   plane out of range, chi^2 with band != -1, a plane the model lacks, the same item twice, nfit > DANGX_MAX_FIT, a failed
 *   allocation.  No component type is refused: the residual involves all of them.
 * dangx_moments_get_fit: stat 0 = mean, 1 = standard deviation sqrt(m2 / (n - ddof)); out [npix] of this shard.
 * dangx_chains_get_fit: rules and statistics of dangx_chains_get_signal.  The section of an item is family 8 FIT (below).
 * A sky-model map is data' - residual with data' fixed, so its std is the residual's std and its mean data' minus the residual's.
 * The global reduced chi^2 trace is dangx_chisq_current.  Not covered: histograms / quantiles, batches, lag-1 or pairs of fit items. */
#define DANGX_MAX_FIT 128
int dangx_moments_fit(dangx_ctx *ctx, int nfit, const int32_t *spec);
int dangx_moments_get_fit(dangx_ctx *ctx, int item, int stat, int ddof, double *out);
int dangx_moments_get_fit_dev(dangx_ctx *ctx, int item, int stat, int ddof, double *out_dev);
/* Batched accumulators of registered pixel planes: the run cut into nbatch consecutive batches of L samples, each with its own
 * (mean, m2), so that burn-in can be discarded AFTER the run and one chain gets a batch-means Monte-Carlo error, a model-free
 * effective sample size and split R-hat.  One launch of k_moments_accum's update per accumulation (DANGX_K_BATCH) behind the
 * others, only when something is registered.  Definitions (dang_amd/csrc/dx_batches_host.h):
 *   with c samples held, sample c + 1 goes to batch c / L as its sample c % L + 1 (Welford; a batch's first sample lands on zeros).
 *   When all nbatch batches are full they are merged in place before the sample is taken (k_batches_merge, one launch): batch i
 *     = batches (2i, 2i+1) folded with Chan's update (w = 1/2, c = L/2), the upper half zeroed, L doubled -- the run length need
 *     not be known.  Merges happen at count = nbatch * batch_len * 2^k.
 *   nfull = count / L full batches, p = count % L samples in the open one; `first` leading batches discarded; B' = nfull - first.
 *   stat 0 mean, 1 std: over the samples [first L, count), open batch included; sqrt(M / (N' - ddof)), N' = B'L + p.
 *   stat 2 MCSE = sqrt(S / (B'(B'-1))), S the M2 of the full batches' means (Welford in batch order).        B' >= 2
 *   stat 3 batch-means ESS = (M_f / (B'L - 1)) / MCSE^2, M_f the folded M2 of the full batches; unclamped.    B' >= 2
 *   stat 4 split R-hat: h = B'/2, the halves are the LAST 2h full batches (an odd B' drops its oldest), each folded to (mu, M);
 *     W, B/n and R-hat as dangx_chains_get's with K = 2, n = hL.  NaN where the element never moved, +inf where only the
 *     half-means differ.                                                                                        h >= 1, hL >= 2
 * dangx_moments_batches: planes[r] = {comp, what, plane} as in dangx_moments_hist; nbatch even, 2 .. DANGX_MAX_BATCHES;
 *   batch_len >= 1 the initial L.  Legal after dangx_moments_begin and before the first dangx_moments_accumulate, independent of
 *   dangx_moments_pairs / _hist / _signals (either order, none drops another); a second call replaces the first (nreg = 0: none),
 *   dangx_moments_begin / _end drop it.  Errors (nothing changes, an earlier registration stays): count > 0, a plane that is not
 *   selected, a template / monopole / hi_fit amplitude, the same plane twice, an odd or out-of-range nbatch, batch_len < 1, nreg >
 *   DANGX_MAX_BATCH_PLANES, a failed allocation.  Memory: [reg][batch][mean | m2][npix] f64 of the library's own, zero-filled =
 *   nreg * nbatch * 16 B * npix (one plane x 16 batches at Nside 1024, 12.6 M pixels: 3.2 GB; the main accumulators take 16 B
 *   * npix per plane).
 * dangx_moments_batches_info: the current L, the number of full batches and the samples in the open batch.
 * dangx_moments_batches_get: out[npix] of this shard.  Errors: nothing registered, reg out of range, a bad stat, first outside
 *   0 .. nfull, too few batches or samples for the stat (named), a bad ddof.
 * dangx_moments_batches_raw: one batch's (mean, m2) planes as they are -- the batch-means trace (either output may be NULL).
 * The _dev forms write device arrays of this shard, asynchronously on the context's stream. */
#define DANGX_MAX_BATCHES 32
#define DANGX_MAX_BATCH_PLANES 32
int dangx_moments_batches(dangx_ctx *ctx, int nreg, const int32_t *planes, int nbatch, int64_t batch_len);
int dangx_moments_batches_info(dangx_ctx *ctx, int64_t *batch_len, int32_t *nfull, int64_t *partial);
int dangx_moments_batches_get(dangx_ctx *ctx, int reg, int stat, int first, int ddof, double *out);
int dangx_moments_batches_get_dev(dangx_ctx *ctx, int reg, int stat, int first, int ddof, double *out_dev);
int dangx_moments_batches_raw(dangx_ctx *ctx, int reg, int batch, double *mean_out, double *m2_out);
int dangx_moments_batches_raw_dev(dangx_ctx *ctx, int reg, int batch, double *mean_out_dev, double *m2_out_dev);
/* Sections: one part of a context's accumulator state, read or written in a packed little-endian layout that does not depend on
 * where the context keeps it -- what saving and restoring a run, and handing a chain's accumulators to another process, are
 * made of (definitions in dang_amd/csrc/dx_section_host.h).  A section is addressed by (family, a, b):
 *   family 0 HEAD    (a, b ignored)  DANGX_SECTION_HEAD_BYTES bytes, host forms only: layout version, count, lag-1 flag, nbatch,
 *                                    the current batch length, the full batches, the fill of the open batch and a 64-bit
 *                                    fingerprint of the registration, with one 64-bit value per part of it: the shard (npix,
 *                                    pix0, nmaps); the selection words with type and nindices of the selected components; the
 *                                    lag-1 flag and the pair list; the histogram planes with lo, hi, nbins, bits (and, once a
 *                                    registration has a per-pixel range, every range kind and map checksum: a list of global
 *                                    ranges hashes as it always did); the signal specs (and, only when angles are registered,
 *                                    the angle specs: a registration without angles hashes as it always did); the batch planes
 *                                    with nbatch
 *   family 1 PLANES  (comp, what)    parts mean, m2 (then prev, first, P when lag-1 is tracked), each [selected planes in T, Q, U
 *                                    order][npix] f64; for a template / monopole / hi_fit member (what 0) its host rows in the
 *                                    same part order, each [selected planes][nbands]
 *   family 2 PAIR    (pair, -)       C[npix] f64
 *   family 3 HIST    (reg, -)        the records as the raw histogram getter lays them out
 *   family 4 SIGNAL  (sig, -)        mean, m2, each [npix] f64
 *   family 5 BATCHES (reg, -)        [nbatch][mean, m2][npix] f64
 *   family 6 HIST_RANGE (reg, -)     lo, hi, each [npix] f64: the range maps of a histogram registration with a per-pixel range.
 *                                    Asking for it of a global-range registration is an error.  A put is refused unless the
 *                                    checksum of its maps is the registration's (on a live context: make the registration and
 *                                    hand in the maps first); a holder takes range kind and checksum over from `like` and
 *                                    receives the maps by this put.  Quantile and mode read-outs over several chains take
 *                                    the maps from ctxs[0] and name this section when a holder there lacks it; N and the
 *                                    rank R-hat need no range values and do not ask for it.
 *   family 7 ANGLE   (ang, -)        Cbar, Sbar, each [npix] f64
 *   family 8 FIT     (item, -)       mean, m2, each [npix] f64 (only a context with fit items has it; their specs enter the
 *                                    fingerprint's signal part only when there are any: a registration without them hashes and
 *                                    saves as it always did)
 * _section_bytes: the payload's size.  _section_get / _put: host arrays, returning after the copy; the _dev forms take device
 * arrays and are asynchronous on the context's stream (the host rows of a template / monopole / hi_fit member: the call waits).
 * Transport is one copy per plane; no kernel is launched.  Every get and put checks `bytes` against _section_bytes.
 * A put overwrites that section of a context with live accumulators.  A put of HEAD is refused, naming what differs, unless its
 * fingerprint is that of this context's registration (make the same registrations first); it sets the count and the batch
 * bookkeeping, and a following dangx_moments_accumulate continues as if the samples had been taken on this context: the lag-1
 * product uses the restored prev, the pair terms the restored means, the batch schedule the restored batch length and fill, the
 * histogram limit the restored count.
 * dangx_moments_begin_like makes ctx a HOLDER: it takes over the registrations of `like` (selection, pairs / lag-1 flag,
 * histograms, signals, angles, fit items, batches; the two contexts must agree in npix / pix0 / nmaps / ncomp / nbands and in the components
 * concerned) and allocates NO accumulators; whatever ctx accumulated or held before is dropped.  A section's device memory
 * (its payload rounded up to 256 bytes; batches at the plane pitch of a live context) is allocated when it is first put.  A
 * holder with lag-1 also takes a PLANES payload of the first two parts (mean, m2) alone.  The read-outs over several chains
 * below accept holders at any position; every single-context entry point of this group except _count, _batches_info, _end and
 * the ones here refuses a holder by name.  dangx_moments_held_bytes: the device bytes a holder holds (0 for a live context).
 * Not covered: merging a section into live accumulators, chains of one process on different devices. */
#define DANGX_SECTION_HEAD_BYTES 104
int dangx_moments_section_bytes(dangx_ctx *ctx, int family, int a, int b, int64_t *bytes);
int dangx_moments_section_get(dangx_ctx *ctx, int family, int a, int b, void *out, int64_t bytes);
int dangx_moments_section_get_dev(dangx_ctx *ctx, int family, int a, int b, void *out_dev, int64_t bytes);
int dangx_moments_section_put(dangx_ctx *ctx, int family, int a, int b, const void *in, int64_t bytes);
int dangx_moments_section_put_dev(dangx_ctx *ctx, int family, int a, int b, const void *in_dev, int64_t bytes);
int dangx_moments_begin_like(dangx_ctx *ctx, dangx_ctx *like);
int dangx_moments_held_bytes(dangx_ctx *ctx, int64_t *bytes);
/* frees the accumulators */
int dangx_moments_end(dangx_ctx *ctx);

/* ---- read-outs over SEVERAL chains: Gelman-Rubin R-hat and pooled posterior summaries ---------------------------------------
 * ctxs[0..nchains) are contexts of ONE device holding the same shard, each with its own chain and its own dangx_moments_*
 * accumulators (the data planes can be shared: dangx_adopt_device_data).  The read-outs combine the per-chain accumulators on the
 * device and write only the map asked for; they touch no accumulator, chain or cache, and a run that never calls them launches
 * what it launched before.  Any of the contexts, ctxs[0] included, may be a HOLDER (dangx_moments_begin_like) given the sections of
 * a chain that ran elsewhere: the result is bit for bit that of the live chain; a read-out that needs a section a holder was not
 * given fails, naming the chain and the section, before anything is written.  Definitions (dang_amd/csrc/dx_chains_host.h), per element, chain k with n_k samples, mean_k and
 * m2_k = sum_t (x_t - mean_k)^2, N = sum n_k:
 *   pooled mean / M2: the chains folded in list order from chain 0's own values, d = mean_k - mu, n' = n + n_k,
 *     mu += d (n_k / n'), M += m2_k + d^2 (n n_k / n') -- every added term >= 0.  Pooled std = sqrt(M / (N - ddof)).
 *   W = (sum_k m2_k) / (K (n - 1));  B/n = sum_k (d_k - dbar)^2 / (K - 1) with d_k = mean_k - mean_0, dbar = (sum d_k) / K;
 *   R-hat = sqrt(((n - 1)/n W + B/n) / W) (Gelman et al., BDA3 eq. 11.4): NaN where no chain ever moved (a masked pixel), +inf
 *     where only the means differ.  These three need equal n_k = n >= 2.
 *   pooled ESS = sum_k ESS_k of dangx_moments_get's stat 3 (every chain must track lag-1; NaN propagates).
 *   pooled pair term C += C_k + d_a d_b (n n_k / n'); covariance = C / (N - ddof), correlation = C / sqrt(M_a M_b).
 *   pooled histogram: bin b = sum_k c_{k,b} in 64-bit integers; N, quantiles and mode by dangx_moments_hist_stat's rules on them.
 * stat of dangx_chains_get / _get_template: 0 = pooled mean, 1 = pooled std, 2 = R-hat, 3 = W, 4 = B/n, 5 = pooled ESS;
 *   of _get_signal: 0-4; of _get_angle: dangx_moments_angles' 0-5; of _get_pair: 0 = covariance, 1 = correlation; of _hist_stat: as dangx_moments_hist_stat.
 * Host forms write host arrays laid out as the single-chain getters lay them out and return after the copy; _dev forms write a
 * packed device array asynchronously.  The kernel runs on ctxs[0]'s stream: before it every other chain's stream records an
 * event that stream waits on, after it that stream records an event the other streams wait on, so a following
 * dangx_moments_accumulate on any chain cannot overwrite what the kernel reads.
 * Errors (message on ctxs[0], naming the chain; nothing is written): nchains outside 2..DANGX_MAX_CHAINS, a context listed twice,
 * contexts on different devices (peer access is not supported), differing npix / pix0 / nmaps, a chain without
 * dangx_moments_begin or without a sample, a (comp, what) plane not selected in some chain, a pair / signal / histogram
 * registration (for a histogram including lo, hi, nbins and bits) that is not the same in every chain, unequal n or n < 2 for
 * stats 2-4, lag-1 missing in some chain for stat 5, a bad ddof. */
#define DANGX_MAX_CHAINS 8
int dangx_chains_get(dangx_ctx *const *ctxs, int nchains, int comp, int what, int stat, int ddof, double *out);
int dangx_chains_get_dev(dangx_ctx *const *ctxs, int nchains, int comp, int what, int stat, int ddof, double *out_dev);
int dangx_chains_get_template(dangx_ctx *const *ctxs, int nchains, int comp, int stat, int ddof, double *ta);
int dangx_chains_get_signal(dangx_ctx *const *ctxs, int nchains, int sig, int stat, int ddof, double *out);
int dangx_chains_get_signal_dev(dangx_ctx *const *ctxs, int nchains, int sig, int stat, int ddof, double *out_dev);
int dangx_chains_get_fit(dangx_ctx *const *ctxs, int nchains, int item, int stat, int ddof, double *out);
int dangx_chains_get_fit_dev(dangx_ctx *const *ctxs, int nchains, int item, int stat, int ddof, double *out_dev);
int dangx_chains_get_angle(dangx_ctx *const *ctxs, int nchains, int ang, int stat, double *out);
int dangx_chains_get_angle_dev(dangx_ctx *const *ctxs, int nchains, int ang, int stat, double *out_dev);
int dangx_chains_get_pair(dangx_ctx *const *ctxs, int nchains, int pair, int stat, int ddof, double *out);
int dangx_chains_get_pair_dev(dangx_ctx *const *ctxs, int nchains, int pair, int stat, int ddof, double *out_dev);
int dangx_chains_hist_stat(dangx_ctx *const *ctxs, int nchains, int reg, int stat, int nq, const double *q, double *out);
int dangx_chains_hist_stat_dev(dangx_ctx *const *ctxs, int nchains, int reg, int stat, int nq, const double *q, double *out_dev);
/* Rank-normalised and folded R-hat (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021) of histogram registration reg, read
 * from the chains' records (k_chains_rank; definitions in dang_amd/csrc/dx_rank_host.h).  The samples of one bin are ties and take
 * the average rank, so the records are a sufficient statistic of the statistic of the BINNED trace: nothing is approximated
 * beyond the bin width.  Unlike stat 2 of dangx_chains_get it needs no finite variance (heavy tails do not hide a difference in
 * location) and its folded form sees chains that agree in the mean and differ in spread.  Per pixel, c[k][b] the counter of chain
 * k and bin b, C[b] = sum_k c[k][b] (64-bit), S = sum_b C[b], cum[b] = sum_{b' < b} C[b']:
 *   score of a non-empty bin: u = 2 cum[b] + C[b] + 1 (twice the mid-rank), u' = min(u, 2S + 2 - u), p = (u' - 0.75) / (2S + 0.5)
 *     (Blom), z[b] = -|Phi^-1(p)| where u' == u, +|Phi^-1(p)| otherwise; |Phi^-1| to 1e-12 absolute.
 *   chain k's (n_k, mean_k, m2_k) of its scores by the weighted Welford update over its non-empty bins in ascending order.
 *   W, B/n and R-hat as for dangx_chains_get from these, where n_0 = .. = n_{K-1} = n >= 2 IN THIS PIXEL; NaN otherwise (the
 *     chains' samples left the range a different number of times), NaN where S = 0 or every sample lies in one bin, +inf where
 *     every chain stayed in one bin and the bins differ.
 *   folded: m = the pooled median bin (dangx_moments_hist_stat's quantile rule at q = 0.5); f[k][e] = c[k][m - e] + c[k][m + e]
 *     (f[k][0] = c[k][m]; terms outside the record are 0); the same statistic with f for c and e = 0 .. nbins-1 for b.
 * stat: 0 = bulk (rank-normalised), 1 = folded, 2 = the larger of the two, the number to report (NaN if either is NaN).
 * out[npix] of this shard.  Not split: the histograms are not batched, drift inside a chain is stat 4 of
 * dangx_moments_batches_get.  Errors as for dangx_chains_hist_stat, and a bad stat; dangx_moments_count may differ between the
 * chains (the rule per pixel decides). */
int dangx_chains_hist_rank(dangx_ctx *const *ctxs, int nchains, int reg, int stat, double *out);
int dangx_chains_hist_rank_dev(dangx_ctx *const *ctxs, int nchains, int reg, int stat, double *out_dev);
/* dangx_moments_batches_get over the chains (k_chains_batches): every chain must hold the same registration, L, nbatch and count
 * (anything else is refused, naming the chain).  stat 0 / 1: pooled over chains and over batches first.., the chains folded in
 * list order from each chain's own fold, sqrt(M / (K N' - ddof)); stat 2: sqrt(sum_k MCSE_k^2) / K; stat 3: sum_k ESS_k; stat 4:
 * split R-hat over the 2K half-chains, W and B/n as for one chain with 2K for K, the half-means referred to half 0 of chain 0. */
int dangx_chains_batches_get(dangx_ctx *const *ctxs, int nchains, int reg, int stat, int first, int ddof, double *out);
int dangx_chains_batches_get_dev(dangx_ctx *const *ctxs, int nchains, int reg, int stat, int first, int ddof, double *out_dev);

/* ---- per-kernel timing with HIP events on the context's stream ----------------- */
int dangx_profile_enable(dangx_ctx *ctx, int on);
int dangx_profile_reset(dangx_ctx *ctx);
int dangx_profile_get(dangx_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
/* the same restricted to the launches of that family that worked on `nplanes` (1: T, Q or U alone; 2: Q+U) planes: the T and
 * Q+U instances of a kernel are different code objects with different costs (bench.py's per-kernel roofline entries).
 * DANGX_ROCTX=1 in the environment additionally wraps every timed launch group in a roctx range named after its family
 * (the ROCm marker library is loaded at run time; `rocprofv3 --marker-trace` shows the ranges). */
int dangx_profile_get_planes(dangx_ctx *ctx, int kernel_id, int nplanes, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
