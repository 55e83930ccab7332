"""Accuracy of the sampler kernels' fp64 exp and log (dang_amd/csrc/dx_math.h: exp_nr, log_pos, and their table forms
-DDX_EXP_TABLE / -DDX_LOG_TABLE) on the device.

A small HIP program that includes dx_math.h is compiled into a temporary directory and run over 8.1e6 exp and 1.1e7 log arguments from
the ranges the kernels use -- beta ln(nu/nu_ref), h nu / (k T), accept-test differences, uniform deviates, frequencies,
temperatures -- uniform and clustered at the table boundaries, at 1 and at the ends of the range.  The results are compared
with numpy.longdouble (x87 extended) references: at most 1 ulp, and the maximum is reported."""
import numpy as np
import pytest

from mathlib_harness import _compile, exp_arguments, log_arguments, ulp_error   # the shared device program and argument sets


@pytest.fixture(scope="module")
def harness():
    """the kernels' build"""
    return _compile([])


@pytest.fixture(scope="module")
def harness_tables():
    """the table forms of exp_nr and log_pos (-DDX_EXP_TABLE -DDX_LOG_TABLE; off in the kernels, see dx_math.h)"""
    return _compile(["-DDX_EXP_TABLE", "-DDX_LOG_TABLE"])


def check_exp(harness, name):
    x = exp_arguments(np.random.default_rng(11))
    assert x.size >= 6_000_000
    y = harness(0, x)
    ref = np.exp(x.astype(np.longdouble))
    e = ulp_error(y, ref)
    worst = int(np.argmax(e))
    print("%s: %d arguments, max %.4f ulp at x = %r, mean %.4f" % (name, x.size, e[worst], x[worst], float(e.mean())))
    assert e.max() <= 1.0
    # saturation: ldexp gives inf above ~709.8 and 0 below ~-745 (|x| < 1.4e9), as the polynomial form does
    big = np.array([710.0, 800.0, 1e4, 1e6, 1e8, 1.3e9, -746.0, -800.0, -1e4, -1e6, -1e8, -1.3e9])
    yb = harness(0, big)
    assert np.all(np.isinf(yb[:6]) & (yb[:6] > 0)) and np.all(yb[6:] == 0.0), yb


@pytest.mark.gpu
def test_exp_nr_within_one_ulp(harness):
    check_exp(harness, "exp_nr")


@pytest.mark.gpu
def test_exp_nr_table_form_within_one_ulp(harness_tables):
    check_exp(harness_tables, "exp_nr (DX_EXP_TABLE)")


def check_log(harness, name):
    x = log_arguments(np.random.default_rng(12))
    assert x.size >= 6_000_000
    y = harness(1, x)
    ref = np.log(x.astype(np.longdouble))
    e = ulp_error(y, ref)
    e = np.where(x == 1.0, np.abs(y) * 1e300, e)   # log 1 = 0 exactly
    worst = int(np.argmax(e))
    print("%s: %d arguments, max %.4f ulp at x = %r, mean %.4f" % (name, x.size, e[worst], x[worst], float(e.mean())))
    assert e.max() <= 1.0
    assert harness(1, np.array([1.0]))[0] == 0.0


@pytest.mark.gpu
def test_log_pos_within_one_ulp(harness):
    check_log(harness, "log_pos")


@pytest.mark.gpu
def test_log_pos_table_form_within_one_ulp(harness_tables):
    check_log(harness_tables, "log_pos (DX_LOG_TABLE)")
