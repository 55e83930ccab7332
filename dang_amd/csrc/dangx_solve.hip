// dangx_solve.hip -- the two linear solvers of the amplitude phase and the seams that expose their operators: cg_search on the
// device (device_cg: the parity path, and groups with global-amplitude members through the mixed operators), the direct solve of
// a group with global-amplitude members (device_schur: orchestration of the Schur passes around the host algebra of
// dx_schur_host.h), the residual of the reference's system at the current state (dangx_amp_residual) and compute_rhs / compute_Ax /
// compute_sample_vector / eval_sed on host vectors.  The operators' kernels live next to their launchers (dangx_amp.hip,
// dangx_mixed.hip, dangx_schur.hip); the context, the model and the reductions in dangx_core.hip.
#include "dx_host.h"

// ======================================================================= kernels

namespace {

// eta(i) = rand_normal(0,1), src/dang_cg_mod.f90:256-262, from the keyed stream
__global__ __launch_bounds__(BLOCK) void k_draw_eta(const Model* __restrict__ Mp, GroupArgs a, double* __restrict__ eta) {
    const Model& M = *Mp;
    const long long SN = (long long)flag_nplanes(a.flag) * M.npix;
    const long long u = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (u >= SN) return;
    const int p = (int)(u / M.npix), i = (int)(u - (long long)p * M.npix), k = flag_map(a.flag, p);
    double u1, u2;
    uniform2(a.seed, a.stream, (unsigned long long)(M.pix0 + i), (uint32_t)k, u1, u2);
    eta[u] = rand_normal(0.0, 1.0, u1, u2);
}

// pack / unpack between c%amplitude and x (initialize_x :1173-1282, unpack_amplitudes :1284-1396)
__global__ __launch_bounds__(BLOCK) void k_pack(const Model* __restrict__ Mp, GroupArgs a, double* __restrict__ x, int unpack) {
    const Model& M = *Mp;
    const long long SN = (long long)flag_nplanes(a.flag) * M.npix;
    const long long u = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (u >= SN) return;
    const int p = (int)(u / M.npix), i = (int)(u - (long long)p * M.npix), k = flag_map(a.flag, p);
    for (int g = 0; g < a.ng; ++g) {
        double* amp = M.comp[a.gc[g]].amp + (long long)(k - 1) * M.npix + i;
        if (unpack) *amp = x[(long long)g * SN + u];
        else x[(long long)g * SN + u] = *amp;
    }
}

// CG vector updates (src/dang_cg_mod.f90:283-305) with block partials of sum(r*r)
//  mode 0: r = b2 - q ; d = r                        -> partial sum(r*r)
//  mode 1: x += alpha*d ; r -= alpha*q               -> partial sum(r*r)
//  mode 2: d = r + beta*d
//  mode 3: b2 = b + f
// entries t >= ndot do not enter the partial sums (replicated global rows on the non-root ranks of a sharded run)
__global__ __launch_bounds__(BLOCK) void k_cg_vec(int mode, long long n, long long ndot, double alpha, double* __restrict__ x,
                                                  double* __restrict__ r, double* __restrict__ d,
                                                  const double* __restrict__ q, const double* __restrict__ b2,
                                                  double* __restrict__ partial) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double rr = 0.0;
    if (t < n) {
        if (mode == 0) {
            const double rv = b2[t] - q[t];
            r[t] = rv; d[t] = rv; rr = (t < ndot) ? rv * rv : 0.0;
        } else if (mode == 1) {
            x[t] = x[t] + alpha * d[t];
            const double rv = r[t] - alpha * q[t];
            r[t] = rv; rr = (t < ndot) ? rv * rv : 0.0;
        } else if (mode == 2) {
            d[t] = r[t] + alpha * d[t];
        } else {
            x[t] = b2[t] + q[t];
        }
    }
    if (partial) {
        __shared__ double sh[BLOCK / 64];
        for (int o = 32; o > 0; o >>= 1) rr += __shfl_down(rr, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = rr;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int w = 0; w < BLOCK / 64; ++w) s += sh[w];
            partial[blockIdx.x] = s;
        }
    }
}

// block partials of sum(u*v)
__global__ __launch_bounds__(BLOCK) void k_dot(const double* __restrict__ u, const double* __restrict__ v, long long n,
                                               long long ndot, double* __restrict__ partial) {
    __shared__ double sh[BLOCK / 64];
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double s = (t < n && t < ndot) ? u[t] * v[t] : 0.0;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double w = 0.0;
        for (int q = 0; q < BLOCK / 64; ++q) w += sh[q];
        partial[blockIdx.x] = w;
    }
}

// block partials of sum((b-q)^2) [row 0] and sum(b^2) [row 1] over the diffuse entries t < ndiff of unmasked units
// (the rows of masked units are zero in A and keep whatever b holds: not part of the solve)
__global__ __launch_bounds__(BLOCK) void k_resid_norm(const Model* __restrict__ Mp, const double* __restrict__ b,
                                                      const double* __restrict__ q, long long ndiff, long long SN,
                                                      double* __restrict__ partial) {
    __shared__ double sh[2][BLOCK / 64];
    const Model& M = *Mp;
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double rr = 0.0, bb = 0.0;
    if (t < ndiff) {
        const long long u = t % SN;
        if (!is_masked(M.mask[u % M.npix])) {
            const double r = b[t] - q[t];
            rr = r * r; bb = b[t] * b[t];
        }
    }
    for (int o = 32; o > 0; o >>= 1) { rr += __shfl_down(rr, o, 64); bb += __shfl_down(bb, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = rr; sh[1][threadIdx.x >> 6] = bb; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) v += sh[threadIdx.x][w];
        partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = v;
    }
}

// eval_sed(band, pix, map_n) over the shard (src/dang_component_mod.f90:778-813)
__global__ __launch_bounds__(BLOCK) void k_eval_sed(const Model* __restrict__ Mp, int comp, int band, int map_n,
                                                    double* __restrict__ out) {
    const Model& M = *Mp;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= M.npix) return;
    const Comp& c = M.comp[comp];
    double t0, t1;
    load_theta(M, c, i, map_n, t0, t1);
    out[i] = comp_sed(M, c, i, map_n, band, sed_prep(c, t0, t1));
}

// ======================================================================= host side

// global rows of x <-> c%template_amplitudes (initialize_x :1244-1279, unpack_amplitudes :1355-1393)
void globals_to_x(dangx_ctx* ctx, const GroupArgs& a, std::vector<double>& xg) {
    xg.assign(std::max(a.nglob, 1), 0.0);
    const int k = plane_set_or_none(a.flag).s1;
    for (int t = 0; t < a.nt; ++t) {
        const int l = a.tc[t];
        dx_fitted_bands(ctx->corr_mask[l], ctx->nfit[l], ctx->hm.nbands, [&](int j, int lf) { xg[a.trow[t] + lf] = ctx->tamp[l][k - 1][j]; });
    }
}
void x_to_globals(dangx_ctx* ctx, const GroupArgs& a, const std::vector<double>& xg) {
    const int k = plane_set_or_none(a.flag).s1;
    for (int t = 0; t < a.nt; ++t) {
        const int l = a.tc[t];
        dx_fitted_bands(ctx->corr_mask[l], ctx->nfit[l], ctx->hm.nbands, [&](int j, int lf) {
            const double v = xg[a.trow[t] + lf];
            if (ctx->desc[l].type == DANGX_TEMPLATE && (a.flag & DANGX_FLAG_QU)) {  // :1380-1382 one amplitude for Q and U
                ctx->tamp[l][1][j] = v; ctx->tamp[l][2][j] = v;
            } else {
                ctx->tamp[l][k - 1][j] = v;
            }
        });
        if (ctx->desc[l].type == DANGX_MONOPOLE)  // update_sky_model: self%offset = c%template_amplitudes(:,1), src/dang_data_mod.f90:357-361
            for (int j = 0; j < ctx->hm.nbands; ++j) ctx->hm.offset[j] = ctx->tamp[l][0][j];
    }
    ctx->dirty = true;
}

// sum(a*b) over n entries -> host (deterministic two-stage reduction)
int device_dot(dangx_ctx* ctx, const double* u, const double* v, long long n, long long ndot, double* out) {
    const unsigned nblk = nblocks(n);
    if (ensure_partial(ctx, nblk)) return 1;
    hipLaunchKernelGGL(k_dot, dim3(nblk), dim3(BLOCK), 0, ctx->stream, u, v, n, ndot, ctx->partial);
    return reduce_to_host(ctx, nblk, out);
}

// the global rows at the tail of a device vector hold this rank's sums: make them the sums over all ranks
int rank_sum_rows(dangx_ctx* ctx, double* tail_dev, int rows) {
    if (!ctx->allreduce || rows <= 0) return 0;
    std::vector<double> h(rows);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), tail_dev, sizeof(double) * rows, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (rank_sum(ctx, h.data(), rows)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(tail_dev, h.data(), sizeof(double) * rows, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// out = A in for a group's vectors [diffuse | global rows]; groups with global-amplitude members use the mixed kernels, and in a
// pixel-sharded run their global rows are summed over the ranks
int apply_A(dangx_ctx* ctx, const GroupArgs& a, long long SN, const double* in, double* out) {
    if (a.nt > 0 ? dx_launch_Ax_mixed(ctx, a, SN, in, out) : dx_launch_Ax(ctx, a, SN, in, out, nullptr)) return 1;
    return a.nt > 0 ? rank_sum_rows(ctx, out + SN * a.ng, a.nglob) : 0;
}

// what cg_search starts from (src/dang_cg_mod.f90:179-282), for device_cg and dangx_amp_residual: b2 = compute_rhs (+
// compute_sample_vector(eta) in sample mode) in work[4], x0 = the current amplitudes in work[0], A x0 in work[3]; work[5] (b) and
// work[1] (eta) are scratch.  xg: the global rows of x0.  n = SN * a.ng + a.nglob entries, the work vectors allocated.
int solve_prologue(dangx_ctx* ctx, const GroupArgs& a, long long SN, long long n, std::vector<double>& xg) {
    const bool mixed = a.nt > 0;
    double *x = ctx->work[0], *eta = ctx->work[1], *q = ctx->work[3], *b2 = ctx->work[4], *b = ctx->work[5];
    hipStream_t st = ctx->stream;
    // b = compute_rhs
    if (mixed ? dx_launch_rhs_mixed(ctx, a, SN, b) : dx_launch_rhs(ctx, a, SN, b)) return 1;
    if (mixed && rank_sum_rows(ctx, b + SN * a.ng, a.nglob)) return 1;
    if (a.ml_mode == DANGX_ML_SAMPLE) {  // b2 = b + compute_sample_vector(eta)
        hipLaunchKernelGGL(k_draw_eta, dim3(nblocks(SN)), dim3(BLOCK), 0, st, ctx->dm, a, eta);
        if (mixed ? dx_launch_sv_mixed(ctx, a, SN, eta, q) : dx_launch_sample_vector(ctx, a, SN, eta, q)) return 1;
        if (mixed && rank_sum_rows(ctx, q + SN * a.ng, a.nglob)) return 1;
        hipLaunchKernelGGL(k_cg_vec, dim3(nblocks(n)), dim3(BLOCK), 0, st, 3, n, n, 0.0, b2, nullptr, nullptr, q, b, nullptr);
    } else {
        HIPCHK(ctx, hipMemcpyAsync(b2, b, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    }
    // x0 = current amplitudes (the reference keeps self%x; identical as amplitudes only change via unpack)
    if (a.ng) hipLaunchKernelGGL(k_pack, dim3(nblocks(SN)), dim3(BLOCK), 0, st, ctx->dm, a, x, 0);
    if (mixed) {
        globals_to_x(ctx, a, xg);
        HIPCHK(ctx, hipMemcpyAsync(x + SN * a.ng, xg.data(), sizeof(double) * a.nglob, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    return apply_A(ctx, a, SN, x, q);
}

}  // namespace

// cg_search on the device, src/dang_cg_mod.f90:179-324.  work[0]=x, [1]=r, [2]=d, [3]=q, [4]=b2, [5]=eta/b.
// Groups with global-amplitude members use the mixed kernels; their vectors are [diffuse | global rows].
int device_cg(dangx_ctx* ctx, const GroupArgs& a, int i_max, double converge, int* iters) {
    const long long SN = (long long)flag_planes_h(a.flag) * ctx->hm.npix;
    const long long n = SN * a.ng + a.nglob;
    // pixel-sharded run: the diffuse entries are this rank's, the global rows are replicated (and summed over ranks
    // wherever an operator produces them); dot products count the global rows on the root rank only
    const long long ndot = ctx->is_root ? n : SN * a.ng;
    if (ensure_work(ctx, n)) return 1;
    if (ensure_partial(ctx, nblocks(n))) return 1;
    double *x = ctx->work[0], *r = ctx->work[1], *d = ctx->work[2], *q = ctx->work[3], *b2 = ctx->work[4];
    hipStream_t st = ctx->stream;
    std::vector<double> xg;
    if (solve_prologue(ctx, a, SN, n, xg)) return 1;
    hipLaunchKernelGGL(k_cg_vec, dim3(nblocks(n)), dim3(BLOCK), 0, st, 0, n, ndot, 0.0, x, r, d, q, b2, ctx->partial);
    double delta_new = 0.0, delta_old, dq = 0.0;
    if (reduce_to_host(ctx, nblocks(n), &delta_new) || rank_sum(ctx, &delta_new, 1)) return 1;
    int i = 1;
    while (i < i_max && delta_new > converge) {
        if (apply_A(ctx, a, SN, d, q)) return 1;
        if (device_dot(ctx, d, q, n, ndot, &dq) || rank_sum(ctx, &dq, 1)) return 1;
        const double alpha = delta_new / dq;
        if (ensure_partial(ctx, nblocks(n))) return 1;
        {
            Timed t(ctx, DANGX_K_CG_VEC);
            hipLaunchKernelGGL(k_cg_vec, dim3(nblocks(n)), dim3(BLOCK), 0, st, 1, n, ndot, alpha, x, r, d, q, b2, ctx->partial);
        }
        delta_old = delta_new;
        if (reduce_to_host(ctx, nblocks(n), &delta_new) || rank_sum(ctx, &delta_new, 1)) return 1;
        const double beta = delta_new / delta_old;
        {
            Timed t(ctx, DANGX_K_CG_VEC);
            hipLaunchKernelGGL(k_cg_vec, dim3(nblocks(n)), dim3(BLOCK), 0, st, 2, n, n, beta, x, r, d, q, b2, nullptr);
        }
        i = i + 1;
    }
    if (a.ng) hipLaunchKernelGGL(k_pack, dim3(nblocks(SN)), dim3(BLOCK), 0, st, ctx->dm, a, x, 1);
    if (a.nt > 0) {
        HIPCHK(ctx, hipMemcpyAsync(xg.data(), x + SN * a.ng, sizeof(double) * a.nglob, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        x_to_globals(ctx, a, xg);
    }
    if (iters) *iters = i;
    return 0;
}

// Direct solve of a group with global-amplitude members: eliminate every (pixel, plane) block on the device
// (pass 1), solve the nglob x nglob Schur system on the host, back-substitute per unit (pass 2).  The linear
// system is the one cg_search iterates on (compute_rhs / compute_Ax / compute_sample_vector,
// src/dang_cg_mod.f90:326-1096), quirks included; the answer is its exact solution instead of the iterate at i_max.
// cs[0..nc): the contexts of this process that share the sky (shard order; nc = 1: dangx_amp_sample); as[r], SNs[r]: the
// group as context r sees it.  Row sums are added over the contexts in shard order, then over the ranks (cs[0]'s callback);
// the small system is solved once and every context gets the same global amplitudes.
// defer: in, non-zero: the caller can run the back-substitution itself (together with the sweeps that follow: the plane-set kernel's
// solve on the data minus the templates' new signal); out, non-zero: the new global amplitudes are in the model of every context
// and pass 2 has NOT run -- granted only for a well-conditioned system, whose residual check is skipped (see below).
int device_schur(dangx_ctx* const* cs, int nc, const GroupArgs* as, const long long* SNs, int64_t* n_not_spd, int* nullity, int* defer) {
    dangx_ctx* ctx = cs[0];
    const GroupArgs& a = as[0];
    const int R = a.nglob;
    auto each = [&](auto&& fn) -> int {  // fn(context, its group, its SN) on every context; the first error is the call's
        for (int r = 0; r < nc; ++r)
            if (fn(cs[r], as[r], SNs[r])) { if (cs[r] != ctx) ctx->err = cs[r]->err; return 1; }
        return 0;
    };
    // rows_dev of every context -> host, added in shard order, then over the ranks
    auto gather = [&](std::vector<double>& rows, int n) -> int {
        std::vector<double> part((size_t)n);
        std::fill(rows.begin(), rows.end(), 0.0);
        for (int r = 0; r < nc; ++r) {
            (void)hipSetDevice(cs[r]->device);
            HIPCHK(ctx, hipMemcpyAsync(part.data(), cs[r]->work[0], sizeof(double) * n, hipMemcpyDeviceToHost, cs[r]->stream));
            HIPCHK(ctx, hipStreamSynchronize(cs[r]->stream));
            for (int q = 0; q < n; ++q) rows[q] += part[q];
        }
        return rank_sum(ctx, rows.data(), n);
    };
    auto set_globals = [&](const std::vector<double>& g, bool back_substitute) -> int {  // new global amplitudes (+ pass 2) everywhere
        return each([&](dangx_ctx* c, const GroupArgs& ga, long long SN) -> int {
            (void)hipSetDevice(c->device);
            x_to_globals(c, ga, g);
            return sync_model(c) || (back_substitute && dx_launch_schur_pass2(c, ga, SN));
        });
    };
    // 1. the rows
    if (R > DX_MAX_ROWS) return fail(ctx, "more than 32 global amplitudes in one CG group: use DANGX_SOLVER_CG");
    unsigned corr[MAXT];
    int nfit[MAXT];
    for (int t = 0; t < a.nt; ++t) { corr[t] = ctx->corr_mask[a.tc[t]]; nfit[t] = ctx->nfit[a.tc[t]]; }
    const SchurArgs sa = dx_schur_rows(a.nt, a.trow, corr, nfit, ctx->hm.nbands);
    // 2. pass 1, enqueued on every device before any result is awaited
    const int nrows = R * R + 3 * R;
    if (each([&](dangx_ctx* c, const GroupArgs& ga, long long SN) -> int {
            (void)hipSetDevice(c->device);
            return ensure_work(c, std::max<long long>(nrows, 1)) || dx_launch_schur_pass1(c, ga, sa, SN, c->work[0]);
        }))
        return 1;
    // 3. its rows: S [R][R], t [R], the fluctuation sums [R], G's diagonal [R]; every context / rank then solves the same small system
    std::vector<double> rows(nrows);
    if (gather(rows, nrows)) return 1;
    const double *S = rows.data(), *t = S + (size_t)R * R, *fsum = t + R, *diag = fsum + R;
    unsigned long long bad_all = 0;
    for (int r = 0; r < nc; ++r) {
        unsigned long long bad = 0;
        (void)hipSetDevice(cs[r]->device);
        HIPCHK(ctx, hipMemcpyAsync(&bad, cs[r]->counters, sizeof(bad), hipMemcpyDeviceToHost, cs[r]->stream));
        HIPCHK(ctx, hipStreamSynchronize(cs[r]->stream));
        bad_all += bad;
    }
    if (n_not_spd) *n_not_spd = (int64_t)bad_all;
    // 4. factor (DxSchurLU: why elimination, why equilibrated, what a vanishing pivot means); nullity is reported through cg_iters
    const std::vector<double> fl = dx_schur_fluct(fsum, R, a.ml_mode, a.fluct, sa);
    std::vector<double> g0;
    globals_to_x(ctx, a, g0);
    const DxSchurLU lu(S, diag, R);
    if (lu.bad_row >= 0)
        return fail(ctx, "global amplitude row " + std::to_string(lu.bad_row) + " of the CG group has no support (template zero or fully masked)");
    if (lu.nonfinite) return fail(ctx, "non-finite entry in the system of the global amplitudes");
    // 5. solve for the correction to the current amplitudes
    std::vector<double> d, g(R);
    lu.solve(dx_schur_rhs(S, t, fl, g0, R), d);
    for (int r = 0; r < R; ++r) g[r] = g0[r] + d[r];
    if (nullity) *nullity = R - lu.rank;
    // 6. well / deferred.
    // A well-conditioned system needs no residual check: the entries of the equilibrated S are differences of per-unit terms of
    // size <= 1 formed to a few ulp, so S is known to ~1e-15 absolute and the solution to ~1e-15 / (smallest pivot) -- the pivots
    // of complete pivoting bound |S^-1| up to the growth factor of an R x R elimination.  With every pivot >= 1e-3 (the diffuse
    // members absorb at most 99.9 % of any global row: a Q/U dust template beside synchrotron and dust; the near-degenerate fits
    // -- a monopole beside the CMB -- have pivots of 1e-6 and below) the global rows' residual is <= 1e-12 of b without the
    // check, which costs one more pass over the group's maps and a host round trip.  DANGX_SCHUR_CHECK=1 measures it always
    // (tests/test_gpu_round4.py compares the two).
    const char* chk = getenv("DANGX_SCHUR_CHECK");
    const double minpiv = lu.minpiv();
    // (Only for `template` members, whose amplitudes are of the size of the data -- tests/test_gpu_round4.py.  The bound is a backward
    // error: relative to the size of a row's terms.  A monopole + hi_fit pair can sit at 1e-15 of its terms and 2e-9 of b with
    // pivots of 1e-2, its amplitudes being 1e7 times the data -- seed 243 of a 300-seed run of tests/test_gpu_fuzz.py, where the
    // measured figure is what the report must carry.  DANGX_SCHUR_SKIP=any extends the skip to every member type, for experiments.)
    const char* skp = getenv("DANGX_SCHUR_SKIP");
    bool templates_only = !(skp && skp[0] == 'a');
    for (int m = 0; templates_only && m < a.nt; ++m) templates_only = ctx->desc[a.tc[m]].type == DANGX_TEMPLATE;
    if (skp && skp[0] == 'a') templates_only = true;
    const bool well = lu.rank == R && minpiv >= 1e-3 && templates_only && !(chk && chk[0] == '1');
    const bool deferred = well && defer && *defer;
    if (defer) *defer = deferred ? 1 : 0;
    // 7. the globals (and pass 2, unless the caller runs it)
    if (set_globals(g, !deferred)) return 1;
    if (well) {  // reported: the a-priori bound, no refinement step
        const double bound = 16.0 * R * 2.220446049250313e-16 / minpiv;
        for (int r = 0; r < nc; ++r) { cs[r]->schur_resid = bound; cs[r]->schur_backward = bound; cs[r]->schur_refine = 0; }
        return 0;
    }
    // 8. Residual check + iterative refinement.  Pass 1 forms S and t as sums of per-unit differences that cancel to the
    // part of a global row the diffuse members do NOT absorb; when they absorb nearly all of it (a fitted monopole
    // beside the CMB) S keeps only a few digits and S g = t is solved for a slightly wrong S.  The true residual of the
    // global rows, r = b - A x evaluated directly at the new state (k_schur_resid: no elimination, no cancellation),
    // drives the correction g += S^-1 r; the diffuse rows are re-solved exactly by pass 2.  The contraction factor is
    // cond(S) * (relative error of S); the loop stops at 1e-12 of the row of b, or when a step no longer helps.
    int refine = 0;
    double prev = INFINITY, resid_b = 0.0, resid_bw = 0.0;
    std::vector<double> rr(3 * R), res(R);
    for (int step = 0; step <= 4; ++step) {
        if (each([&](dangx_ctx* c, const GroupArgs& ga, long long SN) -> int {
                (void)hipSetDevice(c->device);
                return dx_launch_schur_resid(c, ga, sa, SN, c->work[0]);
            }))
            return 1;
        if (gather(rr, 3 * R)) return 1;
        const DxSchurNorms nm = dx_schur_norms(rr.data(), fl, R, res);
        if (step > 0 && !(nm.worst < prev)) {  // the last correction did not help: take it back
            for (int r = 0; r < R; ++r) g[r] -= d[r];
            if (set_globals(g, true)) return 1;
            refine -= 1;
            break;
        }
        resid_b = prev = nm.worst;
        resid_bw = nm.worst_bw;
        if (nm.worst <= 1e-12 || nm.worst_bw <= 1e-15 || step == 4) break;
        lu.solve(res, d);
        for (int r = 0; r < R; ++r) g[r] += d[r];
        if (set_globals(g, true)) return 1;
        refine += 1;
    }
    for (int r = 0; r < nc; ++r) { cs[r]->schur_resid = resid_b; cs[r]->schur_backward = resid_bw; cs[r]->schur_refine = refine; }
    return 0;
}

// ======================================================================= C ABI

// the group, its sizes and its work vectors, for a seam that takes (group, flag)
static int seam_common(dangx_ctx* ctx, int group, int flag, GroupArgs& a, long long& SN, long long& n) {
    (void)hipSetDevice(ctx->device);
    if (make_group(ctx, group, flag, a) || sync_model(ctx)) return 1;
    SN = (long long)flag_planes_h(flag) * ctx->hm.npix;
    n = SN * a.ng + a.nglob;
    if (ensure_work(ctx, n)) return 1;
    return 0;
}

extern "C" {

int64_t dangx_group_size(dangx_ctx* ctx, int group, int flag) {
    GroupArgs a;
    if (!ctx || make_group(ctx, group, flag, a)) return -1;
    return (int64_t)a.ng * flag_planes_h(flag) * ctx->hm.npix + a.nglob;
}

int dangx_schur_info(dangx_ctx* ctx, double* rel_residual, int* refinements) {
    if (!ctx) return 1;
    if (rel_residual) { rel_residual[0] = ctx->schur_resid; rel_residual[1] = ctx->schur_backward; }
    if (refinements) *refinements = ctx->schur_refine;
    return 0;
}

int dangx_amp_residual(dangx_ctx* ctx, int group, int flag, int ml_mode, uint64_t seed, uint64_t stream, double* out) {
    if (!ctx || !out) return 1;
    (void)hipSetDevice(ctx->device);
    if (ml_mode != DANGX_ML_SAMPLE && ml_mode != DANGX_ML_OPTIMIZE) return fail(ctx, "bad ml_mode");
    GroupArgs a; long long SN, n;
    if (seam_common(ctx, group, flag, a, SN, n)) return 1;
    a.ml_mode = ml_mode; a.fluct = DANGX_FLUCT_REFERENCE; a.seed = seed; a.stream = stream;
    const long long ndiff = SN * a.ng;
    double *q = ctx->work[3], *b2 = ctx->work[4];
    hipStream_t st = ctx->stream;
    std::vector<double> xg;
    if (solve_prologue(ctx, a, SN, n, xg)) return 1;
    double sums[2] = {0.0, 0.0};
    if (ndiff > 0) {
        const unsigned nblk = nblocks(ndiff);
        if (ensure_partial(ctx, 2ll * nblk)) return 1;
        hipLaunchKernelGGL(k_resid_norm, dim3(nblk), dim3(BLOCK), 0, st, ctx->dm, b2, q, ndiff, SN, ctx->partial);
        if (rows_to_host(ctx, nblk, 2, sums) || rank_sum(ctx, sums, 2)) return 1;
    }
    double worst = 0.0;
    if (a.nglob > 0) {
        std::vector<double> bg(a.nglob), qg(a.nglob);
        HIPCHK(ctx, hipMemcpyAsync(bg.data(), b2 + ndiff, sizeof(double) * a.nglob, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(qg.data(), q + ndiff, sizeof(double) * a.nglob, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int r = 0; r < a.nglob; ++r) {
            const double res = bg[r] - qg[r];
            sums[0] += res * res; sums[1] += bg[r] * bg[r];
            worst = std::max(worst, std::fabs(res) / std::max(std::fabs(bg[r]), 1e-300));
        }
    }
    out[0] = (sums[1] > 0.0) ? std::sqrt(sums[0] / sums[1]) : 0.0;
    out[1] = worst;
    return 0;
}

// ---- secondary seams, host vectors ------------------------------------------------

int dangx_compute_rhs(dangx_ctx* ctx, int group, int flag, double* b) {
    if (!ctx || !b) return 1;
    GroupArgs a; long long SN, n;
    if (seam_common(ctx, group, flag, a, SN, n)) return 1;
    if (a.nt ? dx_launch_rhs_mixed(ctx, a, SN, ctx->work[0]) : dx_launch_rhs(ctx, a, SN, ctx->work[0])) return 1;
    HIPCHK(ctx, hipMemcpyAsync(b, ctx->work[0], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_compute_Ax(dangx_ctx* ctx, int group, int flag, const double* x, double* res) {
    if (!ctx || !x || !res) return 1;
    GroupArgs a; long long SN, n;
    if (seam_common(ctx, group, flag, a, SN, n)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(ctx->work[0], x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (a.nt ? dx_launch_Ax_mixed(ctx, a, SN, ctx->work[0], ctx->work[1]) : dx_launch_Ax(ctx, a, SN, ctx->work[0], ctx->work[1], nullptr)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(res, ctx->work[1], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_compute_sample_vector(dangx_ctx* ctx, int group, int flag, const double* eta, double* res) {
    if (!ctx || !eta || !res) return 1;
    GroupArgs a; long long SN, n;
    if (seam_common(ctx, group, flag, a, SN, n)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(ctx->work[0], eta, sizeof(double) * (size_t)SN, hipMemcpyHostToDevice, ctx->stream));
    if (a.nt ? dx_launch_sv_mixed(ctx, a, SN, ctx->work[0], ctx->work[1]) : dx_launch_sample_vector(ctx, a, SN, ctx->work[0], ctx->work[1])) return 1;
    HIPCHK(ctx, hipMemcpyAsync(res, ctx->work[1], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_eval_sed(dangx_ctx* ctx, int comp, int band, int map_n, double* out) {
    if (!ctx || !out || check_comp(ctx, comp)) return 1;
    (void)hipSetDevice(ctx->device);
    if (band < 0 || band >= ctx->dims.nbands || map_n < 1 || map_n > ctx->dims.nmaps) return fail(ctx, "bad band/map");
    if (sync_model(ctx) || ensure_work(ctx, ctx->hm.npix)) return 1;
    hipLaunchKernelGGL(k_eval_sed, dim3(nblocks(ctx->hm.npix)), dim3(BLOCK), 0, ctx->stream, ctx->dm, comp, band, map_n, ctx->work[0]);
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->work[0], sizeof(double) * (size_t)ctx->hm.npix, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
