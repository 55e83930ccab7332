"""A dense, extended-precision reference for the direct (Schur complement) solve of CG groups with global-amplitude members.

The oracle restates the reference's OPERATORS (compute_rhs / compute_Ax / compute_sample_vector) but has no direct solve of such
a group, so the solve's VALUES had only residual checks.  At Nside 4 the system is small enough to write down: A column by
column from compute_Ax, b from compute_rhs (+ the sample vector), solved in float64 on the equilibrated matrix and refined with
residuals formed in np.longdouble.  Pure numpy; nothing here touches the GPU.

Everything after dense_system works on the LIVE sub-system (masked pixels give all-zero rows and columns) and assumes no symmetry
(a fitted monopole has row weight 1, src/dang_cg_mod.f90:857).

The tolerance of a value check is derived, not tuned: forward_bound(A, x, b, EPS) is the first-order change of the solution when
every entry of A and b moves by a relative EPS.  The GPU and the oracle evaluate SEDs to TOL_SED of each other; an entry of A is
a product of two SED values and an entry of b holds one, hence 2 * TOL_SED, plus 64 ulp for the sums themselves."""
import numpy as np

from util import TOL_SED

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double (x86-64)"
EPS = 2.0 * TOL_SED + 64.0 * 2.2e-16


def dense_matrix(orc, group, flag):
    """A[:, k] = compute_Ax(e_k), in the layout of initialize_x: [diffuse members | global rows]."""
    n = orc.group_size(group, flag)
    A = np.empty((n, n))
    e = np.zeros(n)
    for k in range(n):
        e[k] = 1.0
        A[:, k] = orc.compute_Ax(group, flag, e)
        e[k] = 0.0
    return A


def dense_rhs(orc, group, flag, ml_mode, seed, stream):
    """compute_rhs, plus compute_sample_vector of the oracle's eta for (seed, stream) in `sample` mode -- the reference's quirks
    (the running row counter of its fluctuation term among them) included."""
    b = orc.compute_rhs(group, flag).copy()
    if ml_mode == "sample":
        b = b + orc.compute_sample_vector(group, flag, orc.draw_eta(flag, seed, stream))
    return b


def dense_system(orc, group, flag, ml_mode, seed, stream):
    """(A, b, live) of the system cg_search iterates on.  live: indices of the rows of A that are not all zero (masked pixels)."""
    A = dense_matrix(orc, group, flag)
    b = dense_rhs(orc, group, flag, ml_mode, seed, stream)
    live = np.flatnonzero(np.abs(A).sum(axis=1) > 0)
    return A, b, live


def _equilibrated(A):
    d = np.abs(np.diag(A))
    assert np.all(d > 0) and np.all(np.isfinite(A)), "live system with an empty diagonal entry"
    s = 1.0 / np.sqrt(d)
    return s, A * s[:, None] * s[None, :]


def equilibrated_inverse(A):
    """(s, inverse of the equilibrated matrix) in float64: A^-1 = diag(s) inv diag(s).  solve_extended and forward_bound take it
    as `fact` where several right-hand sides share one matrix."""
    s, As = _equilibrated(A)
    return s, np.linalg.inv(As)


def solve_extended(A, b, max_steps=40, fact=None):
    """Solution of A x = b as longdouble, and |last correction| per element (the reference's own uncertainty).
    Equilibrated with 1/sqrt(|diag|) (the raw matrix of a group with hi_fit members has a 2-norm condition number of ~1e18, the
    equilibrated one ~1e7), solved in float64, refined with residuals formed in longdouble until the correction stops shrinking.
    b may be a matrix of right-hand sides."""
    s, inv = fact if fact is not None else equilibrated_inverse(A)
    Al, bl = A.astype(LD), np.asarray(b).astype(LD)
    sc = s if bl.ndim == 1 else s[:, None]

    def apply_inv(r):   # A^-1 r = s * As^-1 * (s * r), the float64 part of a step
        return (sc * (inv @ (sc * r).astype(np.float64))).astype(LD)

    def size(d, x):     # in the equilibrated unknowns, where no row dominates by its units
        return float(np.abs(d / sc).max() / max(np.abs(x / sc).max(), LD(1e-300)))

    x = apply_inv(bl)
    last, prev = np.abs(x), np.inf
    for _ in range(max_steps):
        d = apply_inv(bl - Al @ x)
        now = size(d, x)
        if not now < 0.5 * prev:    # the correction no longer shrinks: x is at the floor of this arithmetic
            break
        x, last, prev = x + d, np.abs(d), now
        if now == 0.0:
            break
    return x, last


def forward_bound(A, x, b, eps, fact=None):
    """eps * |A^-1| (|A||x| + |b|), per element: the first-order bound on the change of the solution when every entry of A and b
    moves by a relative eps."""
    s, inv = fact if fact is not None else equilibrated_inverse(A)
    ainv = np.abs(inv) * s[:, None] * s[None, :]
    x = np.abs(np.asarray(x, dtype=np.float64))
    return eps * (ainv @ (np.abs(A) @ x + np.abs(b)))


def componentwise_backward_error(A, x, b):
    """max_i |b - A x|_i / (|A||x| + |b|)_i, the residual formed in longdouble."""
    Al, xl, bl = A.astype(LD), np.asarray(x).astype(LD), np.asarray(b).astype(LD)
    r = np.abs(bl - Al @ xl)
    scale = np.abs(Al) @ np.abs(xl) + np.abs(bl)
    return float((r / scale).max())


def schur_complement(A, nrows):
    """Schur complement of the last `nrows` rows, S = A22 - A21 A11^-1 A12, in longdouble."""
    m = A.shape[0] - nrows
    if m == 0:
        return A.astype(LD)
    X, _ = solve_extended(A[:m, :m], A[:m, m:])
    return A[m:, m:].astype(LD) - A[m:, :m].astype(LD) @ X


def schur_pivots(A, nrows):
    """|pivots| that the host solve of the global rows sees, in elimination order: the Schur complement of the last `nrows` rows
    in longdouble, scaled on both sides by 1/sqrt of the global block's diagonal (its value BEFORE elimination), eliminated with
    complete pivoting."""
    m = A.shape[0] - nrows
    S = schur_complement(A, nrows)
    sc = 1.0 / np.sqrt(np.abs(np.diag(A)[m:])).astype(LD)
    S = S * sc[:, None] * sc[None, :]
    piv = []
    for c in range(nrows):
        sub = np.abs(S[c:, c:])
        pr, pc = np.unravel_index(int(np.argmax(sub)), sub.shape)
        pr, pc = pr + c, pc + c
        if not sub.max() > 0:
            piv.extend([0.0] * (nrows - c))
            break
        S[[c, pr], :] = S[[pr, c], :]
        S[:, [c, pc]] = S[:, [pc, c]]
        piv.append(float(abs(S[c, c])))
        f = S[c + 1:, c] / S[c, c]
        S[c + 1:, c + 1:] -= f[:, None] * S[c, c + 1:][None, :]
    return np.asarray(piv)


def packed_state(state, comps, group, flag, nbands):
    """x in the layout of initialize_x (src/dang_cg_mod.f90:1173-1279) from anything with amplitude(l) / template_amplitudes(l)
    -- `state` is a pair of callables (amplitude map of component l, template amplitudes of component l)."""
    from dang_amd import _lib as L
    amp, tamp = state
    planes = {L.FLAG_T: [0], L.FLAG_Q: [1], L.FLAG_U: [2], L.FLAG_QU: [1, 2]}[flag]
    parts, rows = [], []
    for l, c in enumerate(comps):
        if c.cg_group != group or not c.sample_amplitude:
            continue
        if c.type in ("template", "monopole", "hi_fit"):
            ta = tamp(l)
            rows.extend(ta[planes[0], j] for j in range(nbands) if c.corr[j])
        else:
            parts.append(np.asarray(amp(l))[planes].ravel())
    return np.concatenate(parts + [np.asarray(rows, dtype=np.float64)])
