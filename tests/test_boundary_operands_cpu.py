"""The operands of the values the plane-set chains no longer evaluate twice at their boundaries (dang_amd/csrc/dx_chain.h,
dx_kern_planeset.h), on the CPU: the Planck factors and the SED column of the solve (sed_prep, sed_column) against the beta
chain's chain-invariant factor and first evaluation (chain_finish, RegChain::lnl), and the exponent of the beta chain's closing
evaluation against the T chain's set-up.  Each site's expression is written out as the source has it, operation by operation;
the fp64 results must be the same bits (the device's exp_nr and fast_rcp are one function at both sites, as exp and 1/x here).
The launches themselves are compared with recorded bits in tests/test_gpu_planeset_boundary.py."""
import numpy as np

H_PLANCK = 1.0545726691251021e-34 * 2.0 * 3.141592653589793238462643383279502884197
K_B = 1.3806503e-23


def mbb_z(T):
    z = H_PLANCK / (K_B * T)
    return np.where(z > 1e-4, 1e-4, np.where(z < -1e-4, -1e-4, z))


def test_kept_factors_have_the_chains_operands():
    rng = np.random.default_rng(7)
    n = 200_000
    nu = np.array([20.0 * (857.0 / 20.0) ** (j / 9) for j in range(10)]) * 1e9
    nu_ref = 353.0e9
    lnr = np.log(nu / nu_ref)
    beta = np.concatenate([rng.uniform(0.6, 2.6, n - 4), [0.0, -1.0, 1e-300, 2.6]])
    T = np.concatenate([rng.uniform(4.6, 34.6, n - 4), [1e-9, 1e6, 4.6, 34.6]])
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        # sed_prep (dx_sed.h, DANGX_MBB) and sed_column (dx_kern_fused.h): f = p2 * fast_rcp(exp_nr(p1 * nu_c) - 1.0)
        z_p = mbb_z(T)
        p0, p1, p2 = beta + 1.0, z_p, np.exp(z_p * nu_ref) - 1.0
        f = p2[:, None] * (1.0 / (np.exp(p1[:, None] * nu[None, :]) - 1.0))
        col = f * np.exp(p0[:, None] * lnr[None, :])
        # chain_finish (dx_chain.h, CH_MBB_BETA): F = CDIV(A, CEXP(z * nu_c) - 1.0) = A * fast_rcp(...), sample1 = T
        z = mbb_z(T)
        A = np.exp(z * nu_ref) - 1.0
        Fc = A[:, None] * (1.0 / (np.exp(z[:, None] * nu[None, :]) - 1.0))
        # RegChain::lnl (CH_MBB_BETA): s0 = th + 1.0; e = CEXP(s0 * k1); s = F * e
        s0 = beta + 1.0
        e = np.exp(s0[:, None] * lnr[None, :])
        s = Fc * e
        # chain_finish (CH_MBB_T): F = CEXP((sample0 + 1.0) * lnr), sample0 = the value the beta chain ended on
        Ft = np.exp((beta + 1.0)[:, None] * lnr[None, :])
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(f), bits(Fc))
    assert np.array_equal(bits(col), bits(s))
    assert np.array_equal(bits(e), bits(Ft))
