"""dang_amd -- MI355X-native Gibbs inner loop for the `dang` component-separation sampler.

Only the hot path lives here: HIP kernels + C ABI (csrc/, lib/libdangx.so), the host-side
mirror of the reference's module API (api.py), the posterior summaries accumulated on the device
(posterior.py), pixel sharding / reductions (dist.py) and the synthetic-sky generator used by
tests and bench.py (synth.py).
"""
from . import _lib  # noqa: F401
from .api import (BandInfo, DangCGGroup, DangComps, DangData, DangParams, DangxError, Engine, mask_hi_threshold,  # noqa: F401
                  compute_chisq, convert_maps, fit_band_gain, gibbs_iteration, index_sample_coarse_multi, normalize_bandpass, refresh_host_state, index_means, initialize, return_poltype_flag, sample_calibrators, sample_cg_groups,
                  sample_index_mh_fullsky, sample_spectral_parameters, stream_id, tune_perpixel, fusable_first_sweeps, plan_plane_sets, sky_amp_sample, sky_plane_set_sample)
from .posterior import (default_moment_selection, moments_begin, moments_accumulate, posterior_maps,  # noqa: F401
                        default_moment_pairs, moments_pairs, posterior_pair_maps,
                        default_hist_planes, moments_hist, posterior_quantile_maps, hist_ranges_from_moments,
                        default_signal_specs, moments_signals, posterior_signal_maps,
                        default_angle_specs, moments_angles, posterior_angle_maps, chains_get_angle, chains_angle_maps,
                        default_fit_specs, moments_fit, posterior_fit_maps, chains_get_fit, chains_fit_maps,
                        chains_get, chains_get_template, chains_get_signal, chains_get_pair, chains_hist_stat, open_chain,
                        chains_posterior_maps, chains_pair_maps, chains_quantile_maps, chains_signal_maps, chains_hist_rank, chains_rank_maps,
                        moments_batches, posterior_batch_maps, chains_batches_get, chains_batch_maps,
                        dist_chains, moments_save, moments_load)

__version__ = "0.1.0"
