"""The host algebra of the direct solve of a template group (dang_amd/csrc/dx_schur_host.h, what device_schur in
dang_amd/csrc/dangx_solve.hip runs between its launches) in a stand-alone program under the address and undefined-behaviour
sanitizers: the row tables against tables worked out by hand from the rule of src/dang_cg_mod.f90:970-1094, the fluctuation
vector, the equilibrated LU with complete pivoting on systems whose pivots and solutions are known exactly, and the residual norms
of a refinement step.  No device needed; nothing is loaded into Python under a sanitizer.  tests/test_dense_ref_cpu.py runs the same
program on a real Schur system (host_solve)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from dang_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# "rows nt nbands" + per member "trow corr_mask nfit": nrows, nslots, then rt, rj, ftarget (nrows each, when they fit) and bslot (nbands)
# "fluct nt nbands" + the members + "ml_mode fluct" + nrows hex floats: fl
# "rhs R" + S, t, fl, g0: t + fl - S g0
# "lu R nres" + S, diag + nres residual vectors: "bad_row nonfinite rank minpiv", then d of every residual
# "solve R" + S, t, g0, diag: "bad_row nonfinite rank minpiv", then g = g0 + d -- device_schur's steps 4 and 5 without a fluctuation term
# "norms R" + rr (3R), fl: "worst worst_bw", then res
HOST_MAIN = r"""
#include "dx_schur_host.h"
#include <cstdio>
#include <cstring>
#include <memory>
static bool vec(std::vector<double>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i) if (std::scanf("%la", &v[i]) != 1) return false;
    return true;
}
static void put(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%a", i ? " " : "", v[i]);
    std::printf("\n");
}
static bool members(int nt, std::unique_ptr<int[]>& trow, std::unique_ptr<unsigned[]>& corr, std::unique_ptr<int[]>& nfit) {
    trow.reset(new int[(size_t)nt]); corr.reset(new unsigned[(size_t)nt]); nfit.reset(new int[(size_t)nt]);   // exactly nt long
    for (int t = 0; t < nt; ++t) if (std::scanf("%d %u %d", &trow[t], &corr[t], &nfit[t]) != 3) return false;
    return true;
}
static void report(const DxSchurLU& lu) { std::printf("%d %d %d %a\n", lu.bad_row, lu.nonfinite ? 1 : 0, lu.rank, lu.ok() ? lu.minpiv() : 0.0); }
int main() {
    char mode[8] = {};
    int n = 0, nbands = 0;
    if (std::scanf("%7s %d", mode, &n) != 2) return 2;
    std::unique_ptr<int[]> trow, nfit;
    std::unique_ptr<unsigned[]> corr;
    if (!std::strcmp(mode, "rows") || !std::strcmp(mode, "fluct")) {
        if (std::scanf("%d", &nbands) != 1 || !members(n, trow, corr, nfit)) return 2;
        const SchurArgs sa = dx_schur_rows(n, trow.get(), corr.get(), nfit.get(), nbands);
        if (!std::strcmp(mode, "fluct")) {
            int ml_mode = 0, fluct = 0;
            std::vector<double> fsum;
            if (std::scanf("%d %d", &ml_mode, &fluct) != 2 || sa.nrows > DX_MAX_ROWS || !vec(fsum, (size_t)sa.nrows)) return 2;
            put(dx_schur_fluct(fsum.data(), sa.nrows, ml_mode, fluct, sa));
            return 0;
        }
        std::printf("%d %d\n", sa.nrows, sa.nslots);
        const int shown = sa.nrows <= DX_MAX_ROWS ? sa.nrows : 0;
        for (int r = 0; r < shown; ++r) std::printf("%d ", (int)sa.rt[r]);
        std::printf("\n");
        for (int r = 0; r < shown; ++r) std::printf("%d ", (int)sa.rj[r]);
        std::printf("\n");
        for (int r = 0; r < shown; ++r) std::printf("%d ", (int)sa.ftarget[r]);
        std::printf("\n");
        for (int j = 0; j < nbands; ++j) std::printf("%d ", (int)sa.bslot[j]);
        std::printf("\n");
        return 0;
    }
    const int R = n;
    std::vector<double> S, t, fl, g0, diag, res, d;
    if (!std::strcmp(mode, "rhs")) {
        if (!vec(S, (size_t)R * R) || !vec(t, R) || !vec(fl, R) || !vec(g0, R)) return 2;
        put(dx_schur_rhs(S.data(), t.data(), fl, g0, R));
    } else if (!std::strcmp(mode, "lu")) {
        int nres = 0;
        if (std::scanf("%d", &nres) != 1 || !vec(S, (size_t)R * R) || !vec(diag, R)) return 2;
        const DxSchurLU lu(S.data(), diag.data(), R);
        report(lu);
        for (int q = 0; q < nres; ++q) {
            if (!vec(res, R)) return 2;
            if (!lu.ok()) continue;
            lu.solve(res, d);
            put(d);
        }
    } else if (!std::strcmp(mode, "solve")) {
        if (!vec(S, (size_t)R * R) || !vec(t, R) || !vec(g0, R) || !vec(diag, R)) return 2;
        const DxSchurLU lu(S.data(), diag.data(), R);
        report(lu);
        if (!lu.ok()) return 0;
        lu.solve(dx_schur_rhs(S.data(), t.data(), std::vector<double>(R, 0.0), g0, R), d);
        for (int r = 0; r < R; ++r) d[r] = g0[r] + d[r];
        put(d);
    } else if (!std::strcmp(mode, "norms")) {
        std::vector<double> rr;
        if (!vec(rr, (size_t)3 * R) || !vec(fl, R)) return 2;
        const DxSchurNorms nm = dx_schur_norms(rr.data(), fl, R, res);
        std::printf("%a %a\n", nm.worst, nm.worst_bw);
        put(res);
    } else {
        return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="session")
def schur_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("schur_host")
    src, exe = tmp / "host_main.cpp", tmp / "host_main"
    src.write_text(HOST_MAIN)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dang_amd", "csrc"), "-o", str(exe), str(src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and "sanitize" in r.stdout and ("cannot find" in r.stdout or "unsupported" in r.stdout):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stdout
    return str(exe)


def _exe(exe, text):
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout.splitlines()


def _hex(*arrays):
    return "\n".join(" ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()) for a in arrays) + "\n"


def _floats(line):
    return np.array([float.fromhex(v) for v in line.split()])


def _members(members):
    return "".join("%d %d %d\n" % (trow, sum(1 << j for j in bands), nfit) for trow, bands, nfit in members)


def _rows(exe, members, nbands):
    """members: (trow, fitted bands, nfit) each -> dict(nrows, nslots, rt, rj, ftarget, bslot)"""
    out = _exe(exe, "rows %d %d\n" % (len(members), nbands) + _members(members))
    ints = [[int(v) for v in ln.split()] for ln in out]
    return dict(nrows=ints[0][0], nslots=ints[0][1], rt=ints[1], rj=ints[2], ftarget=ints[3], bslot=ints[4])


def _lu(exe, S, diag, residuals=()):
    S = np.asarray(S, dtype=np.float64)
    out = _exe(exe, "lu %d %d\n" % (S.shape[0], len(residuals)) + _hex(S, diag, *residuals))
    bad, nonfinite, rank, minpiv = out[0].split()
    return dict(bad_row=int(bad), nonfinite=int(nonfinite), rank=int(rank), minpiv=float.fromhex(minpiv), d=[_floats(ln) for ln in out[1:]])


def host_solve(exe, S, t, g0, diag):
    """(g, rank, minpiv) of the real host solve: the correction to g0 from the equilibrated LU of S, added to g0"""
    S = np.asarray(S, dtype=np.float64)
    out = _exe(exe, "solve %d\n" % S.shape[0] + _hex(S, t, g0, diag))
    bad, nonfinite, rank, minpiv = out[0].split()
    assert int(bad) == -1 and int(nonfinite) == 0, out[0]
    return _floats(out[1]), int(rank), float.fromhex(minpiv)


# ---- the row tables.  The rule: row trow + lf is the member's lf-th fitted band (the first nfit bands of its corr mask); the LDS
# slots number the bands that carry a row, in band order; the running counter of compute_sample_vector starts at 0 and goes up by
# one for every (band, member) with corr set, bands outermost -- the sum of (member, band) lands on the row the counter names, and
# is dropped when the member does not fit that band or the counter has left the rows.

OVERLAP = [(0, (0, 1, 2), 3), (3, (1, 3), 2)]      # rows: (0,0) (0,1) (0,2) (1,1) (1,3)
DROPPED = [(0, (0, 1, 2), 2), (2, (3,), 1)]        # member 0 fits two of its three corr bands


def test_rows_of_one_template_on_two_bands(schur_exe):
    assert _rows(schur_exe, [(0, (3, 4), 2)], 5) == dict(nrows=2, nslots=2, rt=[0, 0], rj=[3, 4], ftarget=[0, 1], bslot=[-1, -1, -1, 0, 1])


def test_rows_of_two_templates_on_overlapping_bands(schur_exe):
    """counter: band 0 member 0 -> 0; band 1 member 0 -> 1, member 1 -> 2; band 2 member 0 -> 3; band 3 member 1 -> 4.  Their natural
    rows are 0; 1, 3; 2; 4 -- rows 2 and 3 receive each other's sum"""
    assert _rows(schur_exe, OVERLAP, 4) == dict(nrows=5, nslots=4, rt=[0, 0, 0, 1, 1], rj=[0, 1, 2, 1, 3], ftarget=[0, 1, 3, 2, 4],
                                                 bslot=[0, 1, 2, 3])


def test_rows_of_a_member_with_fewer_fitted_than_corr_bands(schur_exe):
    """counter: band 0 -> 0, band 1 -> 1 (member 0's rows 0 and 1); band 2 member 0 -> 2 but it is the member's third corr band of two
    fitted: no row; band 3 member 1 -> 3, past the three rows: row 2's sum is dropped"""
    assert _rows(schur_exe, DROPPED, 4) == dict(nrows=3, nslots=3, rt=[0, 0, 1], rj=[0, 1, 3], ftarget=[0, 1, -1], bslot=[0, 1, -1, 2])


def test_rows_of_exactly_32_and_of_more(schur_exe):
    """four members on the same eight bands: row 8 t + j, counter 4 j + t"""
    four = [(8 * t, range(8), 8) for t in range(4)]
    assert _rows(schur_exe, four, 8) == dict(nrows=32, nslots=8, rt=[r // 8 for r in range(32)], rj=[r % 8 for r in range(32)],
                                              ftarget=[4 * (r % 8) + r // 8 for r in range(32)], bslot=list(range(8)))
    five = [(8 * t, range(8), 8) for t in range(5)]     # 40 rows do not fit: the count alone, for the caller to refuse
    assert _rows(schur_exe, five, 8) == dict(nrows=40, nslots=0, rt=[], rj=[], ftarget=[], bslot=[-1] * 8)


def test_fluctuation_vector_in_both_modes(schur_exe):
    def fl(members, ml_mode, fluct, fsum):
        text = "fluct %d 4\n" % len(members) + _members(members) + "%d %d\n" % (ml_mode, fluct) + _hex(fsum)
        return list(_floats(_exe(schur_exe, text)[0]))
    fsum = [1.0, 2.0, 4.0, 8.0, 16.0]
    assert fl(OVERLAP, L.ML_CODES["sample"], L.FLUCT_REFERENCE, fsum) == [1.0, 2.0, 8.0, 4.0, 16.0]    # rows 2 and 3 swapped
    assert fl(OVERLAP, L.ML_CODES["sample"], L.FLUCT_CORRECT, fsum) == fsum                              # the natural rows
    assert fl(OVERLAP, L.ML_CODES["optimize"], L.FLUCT_REFERENCE, fsum) == [0.0] * 5
    assert fl(OVERLAP, L.ML_CODES["optimize"], L.FLUCT_CORRECT, fsum) == [0.0] * 5
    assert fl(DROPPED, L.ML_CODES["sample"], L.FLUCT_REFERENCE, fsum[:3]) == [1.0, 2.0, 0.0]            # row 2's sum dropped
    assert fl(DROPPED, L.ML_CODES["sample"], L.FLUCT_CORRECT, fsum[:3]) == fsum[:3]


def test_residual_of_the_current_amplitudes(schur_exe):
    out = _exe(schur_exe, "rhs 2\n" + _hex([[1.0, 2.0], [3.0, 4.0]], [10.0, 20.0], [1.0, 2.0], [1.0, 1.0]))
    assert list(_floats(out[0])) == [8.0, 15.0]                # (10 + 1) - (1 + 2), (20 + 2) - (3 + 4)


# ---- the LU

def test_lu_of_the_hand_made_system_of_the_pivot_test(schur_exe):
    """test_dense_ref_cpu.test_schur_pivots_against_a_hand_made_system: S = [[1 - 1/2, 0], [0, 4 - 1]] beside the diagonal (1, 4) --
    pivots 3/4 and 1/2"""
    S, x = np.array([[0.5, 0.0], [0.0, 3.0]]), np.array([3.0, 0.5])
    lu = _lu(schur_exe, S, [1.0, 4.0], [S @ x, [0.0, 0.0]])
    assert (lu["bad_row"], lu["nonfinite"], lu["rank"]) == (-1, 0, 2) and lu["minpiv"] == 0.5
    assert list(lu["d"][0]) == [3.0, 0.5] and list(lu["d"][1]) == [0.0, 0.0]


def test_lu_leaves_a_free_direction_at_zero(schur_exe):
    """two equal rows and columns.  Scaled by the diagonal (4, 4, 16): [[1, 1, 1], [1, 1, 1], [1, 1, 4]]; the first pivot is the 4, the
    multipliers 1/4 leave 3/4 four times, the second pivot is 3/4 and the third 0: rank 2, and column 0 -- the one the first swap moved
    to the end -- stays free"""
    S = np.array([[4.0, 4.0, 8.0], [4.0, 4.0, 8.0], [8.0, 8.0, 64.0]])
    x = np.array([0.0, 1.0, 2.0])
    lu = _lu(schur_exe, S, [4.0, 4.0, 16.0], [S @ x, -3.0 * (S @ x)])
    assert (lu["bad_row"], lu["nonfinite"], lu["rank"]) == (-1, 0, 2) and lu["minpiv"] == 0.75
    assert list(lu["d"][0]) == [0.0, 1.0, 2.0] and list(lu["d"][1]) == [0.0, -3.0, -6.0]
    assert lu["d"][0][0] == 0.0 and not np.signbit(lu["d"][0][0])


def test_lu_reports_a_row_without_support(schur_exe):
    S = np.eye(3)
    for diag, row in (([1.0, 0.0, 1.0], 1), ([1.0, 2.0, -0.0], 2), ([np.nan, 0.0, 1.0], 0), ([1.0, np.inf, 1.0], 1)):
        lu = _lu(schur_exe, S, diag, [[1.0, 1.0, 1.0]])
        assert (lu["bad_row"], lu["nonfinite"], lu["rank"]) == (row, 0, 0) and lu["d"] == []
    assert _lu(schur_exe, S, [1.0, -2.0, 1.0])["bad_row"] == -1            # the size of the diagonal entry counts


def test_lu_reports_a_non_finite_entry(schur_exe):
    for bad in (np.nan, np.inf):
        S = np.array([[2.0, 0.5], [0.5, bad]])
        lu = _lu(schur_exe, S, [1.0, 1.0], [[1.0, 1.0]])
        assert (lu["bad_row"], lu["nonfinite"]) == (-1, 1) and lu["d"] == []


def test_lu_of_one_row(schur_exe):
    lu = _lu(schur_exe, [[8.0]], [4.0], [[4.0]])                            # scaled: 2, the smallest pivot is capped at 1
    assert (lu["bad_row"], lu["nonfinite"], lu["rank"]) == (-1, 0, 1) and lu["minpiv"] == 1.0 and list(lu["d"][0]) == [0.5]
    lu = _lu(schur_exe, [[1e-11]], [1.0], [[1.0]])                          # below the 1e-10 cut: nothing is solved for
    assert lu["rank"] == 0 and lu["minpiv"] == 1.0 and list(lu["d"][0]) == [0.0]


def test_host_solve_adds_the_correction_to_the_current_amplitudes(schur_exe):
    S, g = np.array([[0.5, 0.0], [0.0, 3.0]]), np.array([3.0, 0.5])
    for g0 in ([0.0, 0.0], [1.0, -1.0], [3.0, 0.5]):
        got, rank, minpiv = host_solve(schur_exe, S, S @ g, g0, [1.0, 4.0])
        assert list(got) == [3.0, 0.5] and rank == 2 and minpiv == 0.5


# ---- the residual norms of a refinement step

def test_residual_norms_of_one_step(schur_exe):
    """rows of b - A x (0.5, -0.25), of b (3, -2), the sizes of their terms (8, 4), fluctuation terms (0.5, -2): residuals 1 and -2.25
    against |3.5| and |-4| -- 0.5625 -- and against 8.5 and 6 -- 0.375"""
    out = _exe(schur_exe, "norms 2\n" + _hex([0.5, -0.25, 3.0, -2.0, 8.0, 4.0], [0.5, -2.0]))
    assert list(_floats(out[0])) == [0.5625, 0.375] and list(_floats(out[1])) == [1.0, -2.25]
    out = _exe(schur_exe, "norms 1\n" + _hex([0.25, 0.0, 0.0], [0.0]))     # an empty row of b: the 1e-300 floor
    assert list(_floats(out[0])) == [0.25 / 1e-300, 0.25 / 1e-300] and list(_floats(out[1])) == [0.25]
