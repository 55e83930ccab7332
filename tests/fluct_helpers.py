"""Helpers of the textbook-fluctuation tests (test_fluct_cpu.py, test_gpu_fluct_fast.py): the per-band normals of
DANGX_FLUCT_CORRECT rebuilt on the host, and the data they perturb.

For unit (global pixel p, plane k) and band j (0-based) the term draws (u1, u2) = uniform2(seed, stream, p, k + 4 * (j + 1)) and
eta_j = sqrt(-2 ln u1) sin(2 pi u2) (dx_rng.h; oracle/dang_oracle.c).  A CORRECT sample on the data d is the OPTIMIZE solve on
d + sigma * eta -- on the temperature plane under band calibration d + gain_j * sigma * eta, because compute_rhs divides the
data by the gain and not by sigma."""
import copy
import math

import numpy as np

from dang_amd import _lib as L

import oracle_ffi as O
from util import MAPN


def flag_planes(flag):
    return (2, 3) if flag == L.FLAG_QU else (MAPN[flag],)


def eta_maps(seed, stream, flag, nb, npix, pix0=0):
    """{plane k: eta[nb, npix]} of one (group, flag) solve with the textbook fluctuation term"""
    out = {}
    for k in flag_planes(flag):
        e = np.empty((nb, npix))
        for j in range(nb):
            for i in range(npix):
                u1, u2 = O.uniform2(seed, stream, pix0 + i, k + 4 * (j + 1))
                e[j, i] = math.sqrt(-2.0 * math.log(u1)) * math.sin(2.0 * math.pi * u2)
        out[k] = e
    return out


def perturbed_data(ddata, solves, seed, pix0=0):
    """A copy of ddata with sig_map + (gain on T) * rms * eta for every (flag, stream) of `solves`"""
    nb, nmaps, npix = ddata.sig_map.shape
    dd = copy.copy(ddata)
    dd.engine = None
    dd.sig_map = np.array(ddata.sig_map, dtype=np.float64, copy=True)
    gain = np.ones(nb) if ddata.gain is None else np.asarray(ddata.gain, dtype=np.float64)
    for flag, stream in solves:
        for k, e in eta_maps(seed, stream, flag, nb, npix, pix0).items():
            g = gain[:, None] if k == 1 else 1.0
            dd.sig_map[:, k - 1, :] += g * ddata.rms_map[:, k - 1, :] * e
    return dd


def unmasked(ddata, flag):
    """boolean [npix]: the units of the flag's planes that the solve writes"""
    return np.asarray(ddata.masks)[flag_planes(flag)[0] - 1] != 0.0
