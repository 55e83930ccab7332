"""The package exports what it exported before the posterior layer moved from dang_amd/api.py to dang_amd/posterior.py, and
dang_amd.api still carries every moved public name as the object posterior.py defines.  No device needed."""
import dang_amd as da
from dang_amd import api, posterior

EXPORTED = """BandInfo DangCGGroup DangComps DangData DangParams DangxError Engine mask_hi_threshold compute_chisq convert_maps fit_band_gain
gibbs_iteration index_sample_coarse_multi normalize_bandpass refresh_host_state index_means initialize return_poltype_flag
sample_calibrators sample_cg_groups sample_index_mh_fullsky sample_spectral_parameters stream_id tune_perpixel fusable_first_sweeps
plan_plane_sets sky_amp_sample sky_plane_set_sample default_moment_selection moments_begin moments_accumulate posterior_maps
default_moment_pairs moments_pairs posterior_pair_maps default_hist_planes moments_hist posterior_quantile_maps default_signal_specs
moments_signals posterior_signal_maps chains_get chains_get_template chains_get_signal chains_get_pair chains_hist_stat open_chain
chains_posterior_maps chains_pair_maps chains_quantile_maps chains_signal_maps chains_hist_rank chains_rank_maps moments_batches
posterior_batch_maps chains_batches_get chains_batch_maps dist_chains moments_save moments_load""".split()

MOVED = """default_moment_selection default_moment_pairs default_hist_planes default_signal_specs moments_begin moments_accumulate moments_pairs
moments_hist moments_signals moments_batches posterior_maps posterior_pair_maps posterior_quantile_maps posterior_batch_maps
posterior_signal_maps chains_posterior_maps chains_pair_maps chains_quantile_maps chains_rank_maps chains_batch_maps chains_signal_maps
chains_get chains_get_template chains_get_signal chains_get_pair chains_hist_stat chains_hist_rank chains_batches_get open_chain
DistChains dist_chains head_unpack head_diff dist_verdict moments_save moments_load GLOBAL_TYPES BATCH_STATS""".split()


def test_the_package_exports_what_it_did():
    assert len(EXPORTED) == 60 and len(set(EXPORTED)) == 60
    for name in EXPORTED:
        assert hasattr(da, name), name
    assert da.Engine is api.Engine and da.__version__


def test_api_carries_every_moved_name():
    assert sorted(MOVED) == sorted(posterior.__all__)
    for name in MOVED:
        assert getattr(api, name) is getattr(posterior, name), name
        if name in EXPORTED:
            assert getattr(da, name) is getattr(posterior, name), name
    assert not hasattr(api, "no_such_name")
