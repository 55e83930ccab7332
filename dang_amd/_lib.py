"""ctypes binding of libdangx.so (the C ABI in include/dangx.h).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible the
product path raises.  The CPU oracle lives in oracle/ and is test infrastructure only.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DANGX_LIB selects another build of the same library (A/B timing of kernel variants on one GPU)
LIB_PATH = os.environ.get("DANGX_LIB") or os.path.join(_HERE, "lib", "libdangx.so")

MAX_BANDS, MAX_COMPS, MAX_IND, MAX_GROUP = 32, 16, 2, 8

# enums (include/dangx.h)
POWERLAW, MBB, FREEFREE, LOGNORMAL, CMB, TCMB, TEMPLATE, MONOPOLE, HIFIT = 1, 2, 3, 4, 5, 6, 7, 8, 9
LNL_CHISQ, LNL_MARGINAL, LNL_PRIOR = 1, 2, 3
PRIOR_GAUSSIAN, PRIOR_UNIFORM, PRIOR_JEFFREYS = 1, 2, 3
ML_SAMPLE, ML_OPTIMIZE = 1, 2
FLAG_T, FLAG_Q, FLAG_U, FLAG_QU = 1, 2, 4, 8
SOLVER_DIRECT, SOLVER_CG = 0, 1
FLUCT_CORRECT, FLUCT_REFERENCE = 0, 1
COARSE_REFERENCE, COARSE_DEGRADED = 0, 1
COARSE_MODEL_CODES = {"reference": COARSE_REFERENCE, "degraded": COARSE_DEGRADED}
A2T, A2F, F2T = 0, 1, 2
UNIT_CODES = {"uK_RJ": 0, "uK_cmb": 1, "MJy/sr": 2}
K_AMP_DIRECT, K_INDEX_MH, K_SKY_CHISQ, K_REDUCE, K_CG_AX, K_CG_VEC, K_AMP_INDEX, K_MOMENTS, K_HIST, K_SIGNAL, K_CHAINS, K_BATCH, K_ANGLE, K_FIT = range(14)
KERNEL_NAMES = {K_AMP_DIRECT: "k_amp_direct", K_INDEX_MH: "k_index_mh", K_SKY_CHISQ: "k_sky_chisq",
                K_REDUCE: "k_reduce", K_CG_AX: "k_Ax", K_CG_VEC: "k_cg_vec", K_AMP_INDEX: "k_amp_index", K_MOMENTS: "k_moments",
                K_HIST: "k_hist", K_SIGNAL: "k_signal", K_CHAINS: "k_chains", K_BATCH: "k_batch", K_ANGLE: "k_angle", K_FIT: "k_fit"}
STAT_CODES = {"mean": 0, "std": 1, "rho1": 2, "ess": 3}
PAIR_STAT_CODES = {"cov": 0, "corr": 1}
MAX_PAIRS = 64
HIST_STAT_CODES = {"quantile": 0, "mode": 1, "n": 2}
RANK_STAT_CODES = {"bulk": 0, "folded": 1, "max": 2}
MAX_HIST, MAX_HIST_Q = 32, 16
HIST_SIGNAL = -1                          # planes[r] = (sig, HIST_SIGNAL, 0): a histogram that reads registered signal sig
MAX_SIGNALS = 64
MAX_ANGLES = 64
# stat of an angle read-out (dangx_moments_get_angle); 'between' over several chains only (dangx_chains_get_angle)
ANGLE_STAT_CODES = {"psi": 0, "psi_std": 1, "R": 2, "C": 3, "S": 4, "between": 5}
MAX_CHAINS = 8
CHAINS_STAT_CODES = {"mean": 0, "std": 1, "rhat": 2, "W": 3, "B": 4, "ess": 5}
BATCH_STAT_CODES = {"mean": 0, "std": 1, "mcse": 2, "ess_bm": 3, "split_rhat": 4}
MAX_BATCHES, MAX_BATCH_PLANES = 32, 32
SEC_HEAD, SEC_PLANES, SEC_PAIR, SEC_HIST, SEC_SIGNAL, SEC_BATCHES, SEC_HIST_RANGE, SEC_ANGLE = range(8)   # family of a section
SECTION_NAMES = ("HEAD", "PLANES", "PAIR", "HIST", "SIGNAL", "BATCHES", "HIST_RANGE", "ANGLE")   # the families every context has
SEC_FIT = 8                               # ... and behind them the family only a context with fit items has (moments_fit)
SECTION_NAMES_ALL = SECTION_NAMES + ("FIT",)
MAX_FIT = 128
FIT_KINDS = ("residual", "chisq")         # what 0, 1 of a fit spec (what, band, plane); band -1 for 'chisq'
# a PLANES section of pixel planes is equal parts: mean and m2, and with lag-1 tracking three more behind them (include/dangx.h)
PLANES_MOMENT_PARTS, PLANES_LAG1_PARTS = 2, 5
SECTION_HEAD_BYTES = 104
SIGNAL_KINDS = ("T", "Q", "U", "P")      # kind 0..3 of a signal spec (comp, band, kind)

TYPE_CODES = {"power-law": POWERLAW, "mbb": MBB, "freefree": FREEFREE, "lognormal": LOGNORMAL, "cmb": CMB, "T_cmb": TCMB,
              "template": TEMPLATE, "monopole": MONOPOLE, "hi_fit": HIFIT}
LNL_CODES = {"chisq": LNL_CHISQ, "marginal": LNL_MARGINAL, "prior": LNL_PRIOR}
PRIOR_CODES = {"gaussian": PRIOR_GAUSSIAN, "uniform": PRIOR_UNIFORM, "jeffreys": PRIOR_JEFFREYS}
ML_CODES = {"sample": ML_SAMPLE, "optimize": ML_OPTIMIZE}


class Dims(C.Structure):
    _fields_ = [("npix", C.c_int32), ("nmaps", C.c_int32), ("nbands", C.c_int32), ("ncomp", C.c_int32),
                ("pix0", C.c_int64), ("npix_global", C.c_int64), ("device", C.c_int32), ("reserved", C.c_int32)]


class CompDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("is_synch", C.c_int32), ("nindices", C.c_int32), ("cg_group", C.c_int32),
                ("sample_amplitude", C.c_int32), ("reserved", C.c_int32), ("nu_ref", C.c_double),
                ("lnl_type", C.c_int32 * MAX_IND), ("prior_type", C.c_int32 * MAX_IND),
                ("gauss_prior", (C.c_double * 2) * MAX_IND), ("uni_prior", (C.c_double * 2) * MAX_IND),
                ("step_size", C.c_double * MAX_IND)]


# every symbol include/dangx.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_D = C.POINTER(C.c_double)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)  # dangx_allreduce_fn

SYMBOLS = {
    "dangx_create": (C.c_int, [C.POINTER(_P), C.POINTER(Dims)]),
    "dangx_destroy": (C.c_int, [_P]),
    "dangx_last_error": (C.c_char_p, [_P]),
    "dangx_version": (C.c_char_p, []),
    "dangx_set_stream": (C.c_int, [_P, _P]),
    "dangx_synchronize": (C.c_int, [_P]),
    "dangx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "dangx_set_host_stride": (C.c_int, [_P, C.c_int64]),
    "dangx_set_allreduce": (C.c_int, [_P, _P, _P, C.c_int]),
    "dangx_index_sample_coarse": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                            C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "dangx_coarse_sizes": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dangx_coarse_partials": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_coarse_chains": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, _P, _P]),
    "dangx_coarse_writeback": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_set_coarse_model": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "dangx_coarse_model_size": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "dangx_coarse_model_partials": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_coarse_model_finish": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_udgrade": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int]),
    "dangx_index_masked_sum": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "dangx_index_plain_sum": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dangx_unit_conversion": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "dangx_normalize_bandpass": (C.c_int, [_P, C.c_int, _P]),
    "dangx_convert_maps": (C.c_int, [_P, _P, _P, _P]),
    "dangx_set_band": (C.c_int, [_P, C.c_int, C.c_double, C.c_int, _P, _P]),
    "dangx_set_component": (C.c_int, [_P, C.c_int, C.POINTER(CompDesc)]),
    "dangx_set_tcmb": (C.c_int, [_P, C.c_double]),
    "dangx_set_calibration": (C.c_int, [_P, _P, _P]),
    "dangx_upload_data": (C.c_int, [_P, _P, _P, _P]),
    "dangx_adopt_device_data": (C.c_int, [_P, _P, _P, _P]),
    "dangx_put_amplitude": (C.c_int, [_P, C.c_int, _P]),
    "dangx_get_amplitude": (C.c_int, [_P, C.c_int, _P]),
    "dangx_put_indices": (C.c_int, [_P, C.c_int, _P]),
    "dangx_get_indices": (C.c_int, [_P, C.c_int, _P]),
    "dangx_set_template": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "dangx_put_template_amplitudes": (C.c_int, [_P, C.c_int, _P]),
    "dangx_get_template_amplitudes": (C.c_int, [_P, C.c_int, _P]),
    "dangx_adopt_device_state": (C.c_int, [_P, C.c_int, _P, _P]),
    "dangx_amplitude_devptr": (_P, [_P, C.c_int]),
    "dangx_indices_devptr": (_P, [_P, C.c_int]),
    "dangx_amp_sample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                   C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "dangx_schur_info": (C.c_int, [_P, _D, C.POINTER(C.c_int)]),
    "dangx_amp_residual": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _D]),
    "dangx_index_sample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                     C.POINTER(C.c_int64)]),
    "dangx_index_sample_pair": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dangx_amp_index_sample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                         C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dangx_plane_set_sample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_double,
                                         C.c_int, _P, _P, _P, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int64), _P]),
    "dangx_plane_sweeps_sample": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_uint64, _P]),
    "dangx_sky_plane_set_sample": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                             C.c_double, C.c_int, _P, _P, _P, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int64), _P]),
    "dangx_sky_model_chisq": (C.c_int, [_P, C.c_int, C.c_int, _D, _P, _P, _P]),
    "dangx_sky_model_chisq_dev": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "dangx_chisq_cached": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _D]),
    "dangx_chisq_current": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "dangx_index_masked_sums": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "dangx_chisq_cached_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_fullsky_prepare": (C.c_int, [_P, C.c_int, C.c_int]),
    "dangx_fullsky_prepare_coarse": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dangx_fullsky_sums": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "dangx_fill_index": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double]),
    "dangx_gain_sums": (C.c_int, [_P, C.c_int, _P]),
    "dangx_peek_indices": (C.c_int, [_P, C.c_int, C.c_int, C.c_longlong, _P]),
    "dangx_fullsky_finish_coarse": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    # the sky-wide steps, chain included: (ctxs, nctx, ...) = the contexts of this process in shard order
    "dangx_fullsky_sample": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                       C.c_int, C.c_int, C.POINTER(C.c_int32), _D, _D, C.POINTER(C.c_int64)]),
    "dangx_tune_step_size": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _D,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_int32), _D]),
    "dangx_tune_perpixel": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                      C.POINTER(C.c_int32), _D]),
    "dangx_fit_band_gain": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _D]),
    "dangx_update_tcmb": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, _D]),
    "dangx_plan_fusion": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "dangx_sky_amp_sample": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                       C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "dangx_group_size": (C.c_int64, [_P, C.c_int, C.c_int]),
    "dangx_compute_rhs": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "dangx_compute_Ax": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "dangx_compute_sample_vector": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "dangx_eval_sed": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_rtc_kernels": (C.c_int, [_P, C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "dangx_rtc_compile": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "dangx_moments_begin": (C.c_int, [_P, _P]),
    "dangx_moments_accumulate": (C.c_int, [_P]),
    "dangx_moments_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "dangx_moments_get": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_get_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_get_template": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_pairs": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "dangx_moments_get_pair": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_get_pair_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_hist": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int]),
    "dangx_moments_hist_get": (C.c_int, [_P, C.c_int, _P]),
    "dangx_moments_hist_get_dev": (C.c_int, [_P, C.c_int, _P]),
    "dangx_moments_hist_stat": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "dangx_moments_hist_stat_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "dangx_moments_hist_range_maps": (C.c_int, [_P, C.c_int, _P, _P]),
    "dangx_moments_hist_range_maps_dev": (C.c_int, [_P, C.c_int, _P, _P]),
    "dangx_moments_hist_range_get": (C.c_int, [_P, C.c_int, _P, _P]),
    "dangx_moments_hist_range_get_dev": (C.c_int, [_P, C.c_int, _P, _P]),
    "dangx_moments_signals": (C.c_int, [_P, C.c_int, _P]),
    "dangx_moments_get_signal": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_get_signal_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_angles": (C.c_int, [_P, C.c_int, _P]),
    "dangx_moments_get_angle": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "dangx_moments_get_angle_dev": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "dangx_moments_fit": (C.c_int, [_P, C.c_int, _P]),
    "dangx_moments_get_fit": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_get_fit_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_end": (C.c_int, [_P]),
    "dangx_moments_batches": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int64]),
    "dangx_moments_batches_info": (C.c_int, [_P, _P, _P, _P]),
    "dangx_moments_batches_get": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_batches_get_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_moments_batches_raw": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "dangx_moments_batches_raw_dev": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    # sections of the accumulator state: (ctx, family, a, b, ...)
    "dangx_moments_section_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "dangx_moments_section_get": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "dangx_moments_section_get_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "dangx_moments_section_put": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "dangx_moments_section_put_dev": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    "dangx_moments_begin_like": (C.c_int, [_P, _P]),
    "dangx_moments_held_bytes": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    # read-outs over several chains: (ctxs, nchains, ...) = one context per chain
    "dangx_chains_get": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_template": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_signal": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_signal_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_fit": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_fit_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_angle": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_angle_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_pair": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_get_pair_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_hist_stat": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "dangx_chains_hist_stat_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "dangx_chains_hist_rank": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_hist_rank_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_batches_get": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_chains_batches_get_dev": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "dangx_profile_enable": (C.c_int, [_P, C.c_int]),
    "dangx_profile_reset": (C.c_int, [_P]),
    "dangx_profile_get": (C.c_int, [_P, C.c_int, _D, C.POINTER(C.c_int64)]),
    "dangx_profile_get_planes": (C.c_int, [_P, C.c_int, C.c_int, _D, C.POINTER(C.c_int64)]),
}

_lib = None


def load():
    """Load libdangx.so and attach prototypes.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libdangx.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'`; "
            "there is no CPU fallback for the product path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
