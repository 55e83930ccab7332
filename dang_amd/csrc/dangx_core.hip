// dangx_core.hip -- the context behind the C ABI of include/dangx.h: creation, the host mirror of the model and its device copy
// (sync_model: band constants, host-evaluated SEDs of spatially constant index maps, bandpass tables), the resident state maps,
// the chi^2 / index-sum ring the sweeps leave their by-products in (chi_next / chi_flush), the CG group descriptors
// (make_group), the small reduction / statistics / unit-conversion entry points and the launch profile.  The two linear solvers
// and the seams of their operators live in dangx_solve.hip, the sampling entry points in dangx_entry.hip, the full-sky / coarse-
// Nside device side in dangx_coarse.hip, the sky-wide chains in dangx_sky.hip, the kernels next to their launchers.
//
// Design: one thread owns one (pixel, Stokes plane) unit -- the reference's global CG system is block diagonal
// for diffuse components, so the amplitude phase is a single streaming pass (mixing rows -> normal equations -> Cholesky) and
// the index phase a single pass with the Metropolis chain held in registers.  All map arrays are pixel-major, so a wavefront's
// 64 lanes read 64 consecutive doubles (512 B) per load.  Everything is fp64.
#include <dlfcn.h>

#include "dx_host.h"

DxRoctx::DxRoctx() {
    const char* e = getenv("DANGX_ROCTX");
    if (!(e && e[0] == '1')) return;
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
        void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
        if (!h) continue;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr; pop = nullptr;
    }
}
const DxRoctx& dx_roctx() {
    static const DxRoctx r;
    return r;
}
const char* dx_kernel_family(int kid) {
    static const char* const names[DANGX_K_COUNT] = {"dangx:amplitude_solve", "dangx:index_sweep", "dangx:sky_chisq", "dangx:reduce",
                                                     "dangx:cg_Ax", "dangx:cg_vec", "dangx:solve+sweeps", "dangx:moments", "dangx:hist",
                                                     "dangx:signal", "dangx:chains", "dangx:batches", "dangx:angle", "dangx:fit"};
    return (kid >= 0 && kid < DANGX_K_COUNT) ? names[kid] : "dangx:?";
}


// ======================================================================= kernels

namespace {

// deterministic second stage: out[0] = sum(partial[0..n)) in a fixed order
__global__ __launch_bounds__(BLOCK) void k_reduce(const double* __restrict__ partial, long long n, double* __restrict__ out) {
    __shared__ double sh[BLOCK];
    double s = 0.0;
    for (long long t = threadIdx.x; t < n; t += BLOCK) s += partial[t];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// first stage of a deterministic row-wise reduction: in[q][0..n) -> out[q][0..gridDim.x), fixed chunking
__global__ __launch_bounds__(BLOCK) void k_reduce_rows(const double* __restrict__ in, long long n, int rows,
                                                       double* __restrict__ out) {
    __shared__ double sh[BLOCK];
    const long long chunk = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    for (int q = 0; q < rows; ++q) {
        double s = 0.0;
        for (long long t = lo + threadIdx.x; t < hi; t += BLOCK) s += in[(long long)q * n + t];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[(long long)q * gridDim.x + blockIdx.x] = sh[0];
        __syncthreads();
    }
}

// second stage for the fused chi^2: cache[0..2] = chi^2 "before" of planes 1..3, cache[3..5] = "after".
// rows of `partial`: before(plane s1), before(plane s2), after(s1), after(s2); write_before = first sweep
// on these planes since the last amplitude update.
__global__ __launch_bounds__(BLOCK) void k_reduce_chi(const double* __restrict__ partial, long long n, int s1, int s2,
                                                      int write_before, double* __restrict__ cache) {
    __shared__ double sh[BLOCK];
    for (int q = 0; q < 4; ++q) {
        double s = 0.0;
        for (long long t = threadIdx.x; t < n; t += BLOCK) s += partial[(long long)q * n + t];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const int plane = (q & 1) ? s2 : s1;
            const bool after = q >= 2;
            if (!((q & 1) && s1 == s2) && (after || write_before)) cache[(after ? 3 : 0) + plane - 1] = sh[0];
        }
        __syncthreads();
    }
}

// the same two stages for up to CHI_RING sweeps at once, in launch order (identical sums: same chunks, same trees)
constexpr int CHI_ROWS = 4 + DX_MAX_IDXSUM;   // rows of a stage entry: the four chi^2 sums + the index sums of a plane-set launch
struct ChiBatch {
    const double* buf[dangx_ctx::CHI_RING];
    long long nblk[dangx_ctx::CHI_RING];
    int s1[dangx_ctx::CHI_RING], s2[dangx_ctx::CHI_RING], wb[dangx_ctx::CHI_RING], ns[dangx_ctx::CHI_RING];
    int slot[dangx_ctx::CHI_RING][DX_MAX_IDXSUM];
    int n;
};
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_batch(ChiBatch b, double* __restrict__ stage) {
    __shared__ double sh[BLOCK];
    const int e = blockIdx.y;
    const double* in = b.buf[e];
    const long long n = b.nblk[e];
    double* out = stage + (long long)e * CHI_ROWS * gridDim.x;
    const long long chunk = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    const int q = blockIdx.z;   // one row per block: the rows of an entry reduce side by side
    if (q >= 4 + b.ns[e]) return;
    double s = 0.0;
    for (long long t = lo + threadIdx.x; t < hi; t += BLOCK) s += in[(long long)q * n + t];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(long long)q * gridDim.x + blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(BLOCK) void k_reduce_chi_batch(ChiBatch b, const double* __restrict__ stage, long long n,
                                                            double* __restrict__ cache) {
    __shared__ double sh[BLOCK];
    const int q = blockIdx.x;   // one row per block; the entries in launch order (a later launch overwrites an earlier one's slot)
    for (int e = 0; e < b.n; ++e) {
        if (q >= 4 + b.ns[e]) continue;   // (block-uniform)
        const double* partial = stage + (long long)e * CHI_ROWS * n;
        double s = 0.0;
        for (long long t = threadIdx.x; t < n; t += BLOCK) s += partial[(long long)q * n + t];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (q >= 4) {   // masked sum of an index map the launch swept: the same value on every plane it wrote (:465)
                for (int k = b.s1[e]; k <= b.s2[e]; ++k) cache[b.slot[e][q - 4] + (k - b.s1[e])] = sh[0];
            } else {
                const int plane = (q & 1) ? b.s2[e] : b.s1[e];
                const bool after = q >= 2;
                if (!((q & 1) && b.s1[e] == b.s2[e]) && (after || b.wb[e])) cache[(after ? 3 : 0) + plane - 1] = sh[0];
            }
        }
        __syncthreads();
    }
}

// fit_band_gain sums (src/dang_sample_mod.f90:590-607): rows 0: sum map2*N_inv*map1, 1: sum map1*N_inv*map1
__global__ __launch_bounds__(BLOCK) void k_gain_rows(const Model* __restrict__ Mp, int band, double* __restrict__ partial) {
    __shared__ double sh[2][BLOCK / 64];
    const Model& M = *Mp;
    const int npix = M.npix;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double v0 = 0.0, v1 = 0.0;
    if (i < npix && !is_masked(M.mask[i])) {
        double sky = 0.0;  // sky_model(i,1,band), update_sky_model order (:355-373)
        for (int l = 0; l < M.ncomp; ++l) {
            const Comp& c = M.comp[l];
            double t0, t1;
            load_theta(M, c, i, 1, t0, t1);
            if (c.type == DANGX_MONOPOLE) continue;
            sky = sky + comp_signal(M, c, i, 1, band, c.amp[i], sed_prep(c, t0, t1));
        }
        const long long q = ((long long)band * M.nmaps) * npix + i;
        const double res = (M.sig[q] - M.offset[band]) / M.gain[band] - sky;  // res_map(i,1,band), :384
        const double noise = M.rms[q];
        const double N_inv = 1.0 / (noise * noise);
        const double map2 = res + sky;
        v0 = map2 * N_inv * sky;
        v1 = sky * N_inv * sky;
    }
    for (int o = 32; o > 0; o >>= 1) { v0 += __shfl_down(v0, o, 64); v1 += __shfl_down(v1, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = v0; sh[1][threadIdx.x >> 6] = v1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += sh[threadIdx.x][w];
        partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// second stage: out[row] = sum(partial[row][0..n))
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_final(const double* __restrict__ partial, long long n, int rows,
                                                             double* __restrict__ out) {
    __shared__ double sh[BLOCK];
    for (int q = blockIdx.x; q < rows; q += gridDim.x) {  // a row is always summed by one block, in one order
        double s = 0.0;
        for (long long t = threadIdx.x; t < n; t += BLOCK) s += partial[(long long)q * n + t];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = BLOCK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[q] = sh[0];
        __syncthreads();
    }
}


// mask_avg / mask_sum (src/dang_util_mod.f90:186-226) of c%indices(:, map_n, nind): rows 0: sum over unmasked pixels,
// 1: their number -- what write_data prints every iteration (src/dang_data_mod.f90:716-731)
__global__ __launch_bounds__(BLOCK) void k_index_masked_sum(const Model* __restrict__ Mp, int comp, int nind, int k,
                                                            double* __restrict__ partial) {
    __shared__ double sh[2][BLOCK / 64];
    const Model& M = *Mp;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double v = 0.0, n = 0.0;
    if (i < M.npix && !is_masked(M.mask[i])) {
        v = M.comp[comp].idx[((long long)nind * M.nmaps + (k - 1)) * M.npix + i];
        n = 1.0;
    }
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_down(v, o, 64); n += __shfl_down(n, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = v; sh[1][threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += sh[threadIdx.x][w];
        partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// the same for several (component, index, map) triples in one launch: every block walks its pixels once (grid stride), reads the
// mask once per pixel and adds that pixel to every entry's sum; rows 2e (sum) and 2e + 1 (count, the same for every e)
struct MeanList { int n; int comp[16], nind[16], k[16]; };
__global__ __launch_bounds__(BLOCK) void k_index_masked_sums(const Model* __restrict__ Mp, MeanList ml, double* __restrict__ partial) {
    __shared__ double sh[17][BLOCK / 64];
    const Model& M = *Mp;
    const double* src[16];
#pragma unroll
    for (int e = 0; e < 16; ++e)
        src[e] = (e < ml.n) ? M.comp[ml.comp[e]].idx + ((long long)ml.nind[e] * M.nmaps + (ml.k[e] - 1)) * M.npix : nullptr;
    double v[16], cnt = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < M.npix; i += (long long)gridDim.x * BLOCK) {
        if (is_masked(M.mask[i])) continue;
        cnt += 1.0;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e < ml.n) v[e] += src[e][i];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (e < ml.n) {
            for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_down(v[e], o, 64);
            if ((threadIdx.x & 63) == 0) sh[e][threadIdx.x >> 6] = v[e];
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) sh[16][threadIdx.x >> 6] = cnt;
    __syncthreads();
    if ((int)threadIdx.x < 2 * ml.n) {
        const int e = threadIdx.x >> 1, r = (threadIdx.x & 1) ? 16 : e;
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += sh[r][w];
        partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// plain sums over EVERY local pixel: rows 0: sum(c%indices(:, k, nind)), 1: sum(masks(:,1)) -- the starting point of the
// step-size tuner in the per-pixel branch, sample(l) = sum(c%indices(:,map_inds(1),l))/sum(mask(:,1))
// (src/dang_sample_mod.f90:344: no mask test on the indices, the mask VALUES are summed)
__global__ __launch_bounds__(BLOCK) void k_index_plain_sum(const Model* __restrict__ Mp, int comp, int nind, int k,
                                                           double* __restrict__ partial) {
    __shared__ double sh[2][BLOCK / 64];
    const Model& M = *Mp;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double v = 0.0, m = 0.0;
    if (i < M.npix) {
        v = M.comp[comp].idx[((long long)nind * M.nmaps + (k - 1)) * M.npix + i];
        m = M.mask[i];
    }
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_down(v, o, 64); m += __shfl_down(m, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = v; sh[1][threadIdx.x >> 6] = m; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += sh[threadIdx.x][w];
        partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// convert_maps, src/dang_data_mod.f90:429-463: sig_map(:,:,j) and rms_map(:,:,j) times conversion(j), on the resident maps
__global__ __launch_bounds__(BLOCK) void k_scale_band(double* __restrict__ sig, double* __restrict__ rms, long long n, double f) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (t < n) { sig[t] = sig[t] * f; rms[t] = rms[t] * f; }
}

// c%indices(:, s1:s2, nind) = value (src/dang_sample_mod.f90:329, 483: every pixel, masked ones too)
__global__ __launch_bounds__(BLOCK) void k_fill_index(const Model* __restrict__ Mp, int comp, int nind, int s1, int s2, double value) {
    const Model& M = *Mp;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= M.npix) return;
    for (int k = s1; k <= s2; ++k) M.comp[comp].idx[((long long)nind * M.nmaps + (k - 1)) * M.npix + i] = value;
}

// bit k of flags[0] is set when plane k+1 of a [nmaps][npix] amplitude map holds a non-zero value
__global__ __launch_bounds__(BLOCK) void k_any_nonzero(const double* __restrict__ amp, long long npix, int nmaps,
                                                       unsigned* __restrict__ flags) {
    for (int k = 0; k < nmaps; ++k) {
        bool nz = false;
        for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < npix; t += (long long)gridDim.x * BLOCK)
            nz = nz || (amp[(long long)k * npix + t] != 0.0);
        if (__ballot(nz) && (threadIdx.x & 63) == 0) atomicOr(flags, 1u << k);
    }
}

// flags bit (q*3 + k) is set when index map q, plane k+1 of an [nind][nmaps][npix] array is NOT spatially
// constant; first[q*3 + k] receives its first element
__global__ __launch_bounds__(BLOCK) void k_not_constant(const double* __restrict__ idx, long long npix, int nmaps, int nind,
                                                        unsigned* __restrict__ flags, double* __restrict__ first) {
    for (int q = 0; q < nind; ++q)
        for (int k = 0; k < nmaps; ++k) {
            const double* m = idx + ((long long)q * nmaps + k) * npix;
            const double m0 = m[0];
            bool diff = false;
            for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < npix; t += (long long)gridDim.x * BLOCK)
                diff = diff || (m[t] != m0);
            if (__ballot(diff) && (threadIdx.x & 63) == 0) atomicOr(flags, 1u << (q * 3 + k));
            if (blockIdx.x == 0 && threadIdx.x == 0) first[q * 3 + k] = m0;
        }
}

// flags bit q is set when index map q of an [nind][3][npix] array differs between the Q and the U plane somewhere
__global__ __launch_bounds__(BLOCK) void k_qu_differ(const double* __restrict__ idx, long long npix, int nind, unsigned* __restrict__ flags) {
    for (int q = 0; q < nind; ++q) {
        const double* mq = idx + ((long long)q * 3 + 1) * npix;
        bool diff = false;
        for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < npix; t += (long long)gridDim.x * BLOCK)
            diff = diff || (mq[t] != mq[npix + t]);
        if (__ballot(diff) && (threadIdx.x & 63) == 0) atomicOr(flags, 1u << q);
    }
}

}  // namespace

// ======================================================================= host side

void dx_reduce_two_stage(dangx_ctx* ctx, const double* partial, long long n, double* stage, double* out_dev) {
    hipLaunchKernelGGL(k_reduce_rows, dim3(DX_RSTAGE), dim3(BLOCK), 0, ctx->stream, partial, n, 1, stage);
    hipLaunchKernelGGL(k_reduce, dim3(1), dim3(BLOCK), 0, ctx->stream, stage, (long long)DX_RSTAGE, out_dev);
}
void dx_reduce_rows_to(dangx_ctx* ctx, const double* partial, unsigned nblk, int rows, double* out_dev) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_reduce_rows_final, dim3(rows < 1024 ? rows : 1024), dim3(BLOCK), 0, ctx->stream, partial, (long long)nblk, rows, out_dev);
}

namespace {


// the bandpass sum of the reference's unit conversions and SEDs: term(nu, tau) at (nu_c, 1) for a delta band, otherwise added up
// over the band's samples (nu0, tau0) in their order; samples with nu0 == 0 are skipped.  A delta band's value is its one term:
// the weight 1 changes no bit of it
template <class F>
double band_sum(const dangx_ctx* ctx, const Band& b, F&& term) {
    if (b.n == 0) return term(b.nu_c, 1.0);
    double sum = 0.0;
    for (int i = 0; i < b.n; ++i) {
        const double nu = ctx->bp_nu0[b.off + i];
        if (nu != 0.0) sum = sum + term(nu, ctx->bp_tau0[b.off + i]);
    }
    return sum;
}

// a2t(bp), src/dang_bp_mod.f90:211-243
double host_a2t(const dangx_ctx* ctx, int j) {
    return band_sum(ctx, ctx->hm.band[j], [&](double nu, double tau) {
        const double y = (nu > 1e7f) ? (H_PLANCK * nu) / (K_B * ctx->hm.tcmb) : (H_PLANCK * nu * 1e9) / (K_B * ctx->hm.tcmb);
        return tau * ((std::exp(y) - 1.0) * (std::exp(y) - 1.0)) / ((y * y) * std::exp(y));
    });
}

// compute_bnu_prime_RJ / compute_bnu_prime, src/dang_bp_mod.f90:160-179 (nu in Hz)
double host_bnu_prime_RJ(double nu) { return 2.0 * K_B * std::pow(nu, 2.0) / std::pow(C_LIGHT, 2.0); }
double host_bnu_prime(double nu, double tcmb) {
    const double y = H_PLANCK * nu / (K_B * tcmb);
    return (2.0 * H_PLANCK * (nu * nu * nu)) / (std::pow(C_LIGHT, 2.0) * (std::exp(y) - 1)) * (std::exp(y) / (std::exp(y) - 1)) * H_PLANCK * nu /
           (K_B * (tcmb * tcmb));
}
// a2f(bp) [MJy/sr / uK_RJ], src/dang_bp_mod.f90:181-209.  `sum*1e14` multiplies by a SINGLE-precision literal: 1e14 is
// not representable in real(4), the factor is 100000000376832 -- kept, it is what the reference's maps are scaled by
double host_a2f(const dangx_ctx* ctx, int j) {
    const double sum = band_sum(ctx, ctx->hm.band[j], [](double nu, double tau) {
        return tau * ((nu > 1e7f) ? host_bnu_prime_RJ(nu) : host_bnu_prime_RJ(nu * 1e9));
    });
    return sum * (double)1e14f;
}
// f2t(bp) [uK_cmb / MJy sr-1], src/dang_bp_mod.f90:245-274
double host_f2t(const dangx_ctx* ctx, int j) {
    const double T = ctx->hm.tcmb;
    return band_sum(ctx, ctx->hm.band[j], [T](double nu, double tau) {
        return tau / ((nu > 1e7f) ? host_bnu_prime(nu, T) : host_bnu_prime(nu * 1e9, T)) * 1.0e-14;
    });
}

// eval_sed for a delta bandpass on the host (src/dang_component_mod.f90:886-1040), used for components whose
// indices are spatially constant on a plane
double host_sed(const Comp& c, double nu, double cmb_cst, double th0, double th1) {
    switch (c.type) {
    case DANGX_POWERLAW: return std::pow(nu / c.nu_ref, th0);
    case DANGX_MBB: {
        const double z = mbb_z(th1);
        return (std::exp(z * c.nu_ref) - 1.0) / (std::exp(z * nu) - 1.0) * std::pow(nu / c.nu_ref, th0 + 1.0);
    }
    case DANGX_FREEFREE: {
        auto g = [&](double v) {
            return std::log(std::exp(5.960 - std::sqrt(3.0) / PI * std::log(1.0 * v / 1.0e9 * std::pow(th0 / 1.0e4, -1.5))) + 2.71828);
        };
        const double r = nu / c.nu_ref;
        return g(nu) / g(c.nu_ref) * (1.0 / (r * r));
    }
    case DANGX_LOGNORMAL: {
        const double l = std::log(nu / (th0 * 1e9)) / th1;
        const double q = c.nu_ref / nu;
        return std::exp(-0.5 * (l * l)) * (q * q);
    }
    case DANGX_CMB: return cmb_cst;
    default: return 0.0;
    }
}

}  // namespace

// ---- host helpers shared with dangx_entry.hip / dangx_coarse.hip / dangx_sky.hip (declared in dx_host.h)

// eval_sed of a diffuse component at band j for index values (t0, t1) on the host: the delta form, or the tau0-weighted sum over
// the band's samples (the expressions sync_model uses for spatially constant indices)
double dx_host_band_sed(dangx_ctx* ctx, int comp, int j, double t0, double t1) {
    const Comp& c = ctx->hm.comp[comp];
    const Band& b = ctx->hm.band[j];
    if (c.type == DANGX_CMB) return host_sed(c, b.nu_c, c.cst[j], t0, t1);
    return band_sum(ctx, b, [&](double nu, double tau) { return tau * host_sed(c, nu, 0.0, t0, t1); });
}

int sync_model(dangx_ctx* ctx) {
    if (!ctx->dirty) return 0;
    Model& M = ctx->hm;
    for (int j = 0; j < M.nbands; ++j)
        if (!ctx->band_set[j]) return fail(ctx, "band " + std::to_string(j) + " not set");
    for (int l = 0; l < M.ncomp; ++l)
        if (!ctx->comp_set[l]) return fail(ctx, "component " + std::to_string(l) + " not set");
    if (!ctx->sig || !ctx->rms || !ctx->mask) return fail(ctx, "map data not uploaded");
    for (int l = 0; l < M.ncomp; ++l)
        if (ensure_state(ctx, l)) return 1;
    M.sig = ctx->sig; M.rms = ctx->rms; M.mask = ctx->mask;
    M.all_delta = 1;
    for (int j = 0; j < M.nbands; ++j) if (M.band[j].n != 0) M.all_delta = 0;
    double nu_hi = 0.0;
    for (int j = 0; j < M.nbands; ++j) nu_hi = std::max(nu_hi, M.band[j].nu_c);
    M.mbb_batch_z = 5.0 * nu_hi / 700.0;
    for (int l = 0; l < M.ncomp; ++l)
        if (ctx->desc[l].type == DANGX_TCMB || is_global_type(ctx->desc[l].type)) M.all_delta = 0;  // generic paths only
    const size_t nbp = ctx->bp_nu0.size();
    if (nbp && ctx->bp_dirty) {
        if (ctx->d_bp_nu0) {
            (void)hipFree(ctx->d_bp_nu0); (void)hipFree(ctx->d_bp_tau0); (void)hipFree(ctx->d_bp_lnr);
            ctx->d_bp_nu0 = ctx->d_bp_tau0 = ctx->d_bp_lnr = nullptr;
        }
        const size_t nbytes = nbp * sizeof(double);
        HIPCHK(ctx, hipMalloc(&ctx->d_bp_nu0, nbytes));
        HIPCHK(ctx, hipMalloc(&ctx->d_bp_tau0, nbytes));
        HIPCHK(ctx, hipMalloc(&ctx->d_bp_lnr, nbytes * M.ncomp));
        // samples with nu0 == 0 are skipped by the reference: on the device they carry tau = 0 and nu = 1 GHz
        std::vector<double> nue(ctx->bp_nu0), taue(ctx->bp_tau0);
        for (size_t q = 0; q < nbp; ++q)
            if (nue[q] == 0.0) { nue[q] = 1.0e9; taue[q] = 0.0; }
        HIPCHK(ctx, hipMemcpy(ctx->d_bp_nu0, nue.data(), nbytes, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(ctx->d_bp_tau0, taue.data(), nbytes, hipMemcpyHostToDevice));
        std::vector<double> lnr(nbp * M.ncomp, 0.0);  // (nu/nu_ref)**beta = exp(beta*log(nu/nu_ref)): the log once, here
        for (int l = 0; l < M.ncomp; ++l)
            for (size_t q = 0; q < nbp; ++q)
                if (ctx->bp_nu0[q] != 0.0) lnr[l * nbp + q] = std::log(ctx->bp_nu0[q] / ctx->desc[l].nu_ref);
        HIPCHK(ctx, hipMemcpy(ctx->d_bp_lnr, lnr.data(), nbytes * M.ncomp, hipMemcpyHostToDevice));
        ctx->bp_dirty = false;
    }
    M.bp_nu0 = ctx->d_bp_nu0; M.bp_tau0 = ctx->d_bp_tau0;
    for (int l = 0; l < M.ncomp; ++l) {
        Comp& c = M.comp[l];
        const dangx_comp_desc& d = ctx->desc[l];
        c.type = d.type; c.nind = d.nindices; c.group = d.cg_group; c.sample_amp = d.sample_amplitude;
        c.is_synch = d.is_synch; c.nu_ref = d.nu_ref;
        c.amp = ctx->amp[l]; c.idx = ctx->idx[l];
        c.tmpl = ctx->tmpl[l]; c.corr_mask = ctx->corr_mask[l]; c.nfit = ctx->nfit[l];
        c.bp_lnr = ctx->d_bp_lnr ? ctx->d_bp_lnr + (size_t)l * nbp : nullptr;
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < MAXB; ++j) c.tamp[k][j] = ctx->tamp[l][k][j];
        if (is_global_type(c.type) && !c.tmpl) return fail(ctx, "global-amplitude component without a template map (dangx_set_template)");
        for (int q = 0; q < MAXI; ++q) {
            c.lnl_type[q] = d.lnl_type[q]; c.prior_type[q] = d.prior_type[q];
            c.gauss[q][0] = d.gauss_prior[q][0]; c.gauss[q][1] = d.gauss_prior[q][1];
            c.uni[q][0] = d.uni_prior[q][0]; c.uni[q][1] = d.uni_prior[q][1];
            c.step[q] = d.step_size[q];
            c.lgden[q] = std::log(d.gauss_prior[q][1] * std::sqrt(2.0 * PI));
        }
        c.lnuref9 = std::log(1.0 * c.nu_ref / 1.0e9);
        for (int j = 0; j < M.nbands; ++j) {
            const double nu = M.band[j].nu_c;
            const double r = nu / c.nu_ref;
            c.lnr[j] = std::log(r);
            c.lnu9[j] = std::log(1.0 * nu / 1.0e9);
            c.cst[j] = 0.0;
            if (c.type == DANGX_CMB) c.cst[j] = 1.0 / host_a2t(ctx, j);
            else if (c.type == DANGX_FREEFREE) c.cst[j] = 1.0 / (r * r);
            else if (c.type == DANGX_LOGNORMAL) { const double q = c.nu_ref / nu; c.cst[j] = q * q; }
        }
        c.const_planes = 0;
        if (c.type >= DANGX_POWERLAW && c.type <= DANGX_CMB) {  // the diffuse types; bandpass bands: the tau0-weighted sum
            const unsigned cp = (c.nind == 0) ? 7u : ctx->idx_const[l];
            for (int k = 0; k < M.nmaps; ++k)
                if ((cp >> k) & 1) {
                    c.const_planes |= 1 << k;
                    const double t0 = ctx->idx_val[l][k][0], t1 = ctx->idx_val[l][k][1];
                    for (int j = 0; j < M.nbands; ++j) c.csed[k][j] = dx_host_band_sed(ctx, l, j, t0, t1);
                }
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->dm, &ctx->hm, sizeof(Model), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->dirty = false;
    return 0;
}

int prof_collect(dangx_ctx* ctx) {
    for (auto& e : ctx->events) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventSynchronize(e.b));
        HIPCHK(ctx, hipEventElapsedTime(&ms, e.a, e.b));
        ctx->prof_ms[e.kid] += ms;
        ctx->prof_n[e.kid] += 1;
        ctx->prof_ms_pl[e.kid][e.planes] += ms;
        ctx->prof_n_pl[e.kid][e.planes] += 1;
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    ctx->events.clear();
    return 0;
}


int ensure_work(dangx_ctx* ctx, long long n) {
    if (n <= ctx->work_cap) return 0;
    for (auto& w : ctx->work) {
        if (w) (void)hipFree(w);
        w = nullptr;
        HIPCHK(ctx, hipMalloc(&w, sizeof(double) * (size_t)n));
    }
    ctx->work_cap = n;
    return 0;
}


constexpr int CHI_RSTAGE = 128;  // blocks of the first reduction stage of the sweeps' chi^2 partials

// reduce every pending sweep's block partials into chi_cache (two launches for all of them, in launch order)
int chi_flush(dangx_ctx* ctx) {
    if (ctx->chi_npend == 0) return 0;
    (void)hipSetDevice(ctx->device);  // the caller may have been working on another context's device
    ChiBatch b;
    b.n = ctx->chi_npend;
    for (int e = 0; e < b.n; ++e) {
        const auto& p = ctx->chi_pend[e];
        b.buf[e] = p.buf; b.nblk[e] = p.nblk; b.s1[e] = p.s1; b.s2[e] = p.s2; b.wb[e] = p.wb; b.ns[e] = p.ns;
        for (int q = 0; q < DX_MAX_IDXSUM; ++q) b.slot[e][q] = p.slot[q];
    }
    for (int e = b.n; e < dangx_ctx::CHI_RING; ++e) {
        b.buf[e] = nullptr; b.nblk[e] = 0; b.s1[e] = b.s2[e] = 1; b.wb[e] = 0; b.ns[e] = 0;
        for (int q = 0; q < DX_MAX_IDXSUM; ++q) b.slot[e][q] = 0;
    }
    {
        Timed t(ctx, DANGX_K_REDUCE);
        int rows = 4;
        for (int e = 0; e < b.n; ++e) rows = std::max(rows, 4 + b.ns[e]);
        hipLaunchKernelGGL(k_reduce_rows_batch, dim3(CHI_RSTAGE, b.n, rows), dim3(BLOCK), 0, ctx->stream, b, ctx->chi_stage);
        hipLaunchKernelGGL(k_reduce_chi_batch, dim3(rows), dim3(BLOCK), 0, ctx->stream, b, ctx->chi_stage, (long long)CHI_RSTAGE, ctx->chi_cache);
    }
    ctx->chi_npend = 0;
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
// the buffer the next sweep writes its chi^2 block partials to ([4][nblk]); flushes first when the ring is full
int chi_next(dangx_ctx* ctx, long long nblk, double** buf) {
    if (ctx->chi_npend == dangx_ctx::CHI_RING && chi_flush(ctx)) return 1;
    auto& p = ctx->chi_pend[ctx->chi_npend];
    if (p.cap < CHI_ROWS * nblk) {
        if (p.buf) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(p.buf); p.buf = nullptr; p.cap = 0; }
        HIPCHK(ctx, hipMalloc(&p.buf, sizeof(double) * (size_t)(CHI_ROWS * nblk)));
        p.cap = CHI_ROWS * nblk;
    }
    p.ns = 0;
    *buf = p.buf;
    return 0;
}

int make_group(dangx_ctx* ctx, int group, int flag, GroupArgs& a) {
    PlaneSet ps;
    if (plane_set_of(ctx, flag, ps)) return 1;
    if (ctx->dims.nmaps < 3 && flag != DANGX_FLAG_T) return fail(ctx, "polarisation flag needs nmaps == 3");
    const unsigned planes = map_bits(ps.map_n);  // planes this (group, flag) works on
    std::memset(&a, 0, sizeof(a));
    a.flag = flag;
    for (int l = 0; l < ctx->hm.ncomp; ++l) {
        const dangx_comp_desc& d = ctx->desc[l];
        if (d.type == DANGX_TEMPLATE || d.type == DANGX_MONOPOLE) a.uc[a.nuc++] = l;
        if (d.cg_group == group && d.sample_amplitude && is_global_type(d.type)) {
            if (a.nt >= MAXT) return fail(ctx, "too many global-amplitude components in CG group");
            if (d.type != DANGX_TEMPLATE && flag != DANGX_FLAG_T)
                return fail(ctx, "hi_fit / monopole components are fitted on plane 1: use CG_POLTYPE T for their group");
            a.tc[a.nt] = l; a.trow[a.nt] = a.nglob; a.nglob += ctx->nfit[l]; ++a.nt;
        } else if (d.cg_group == group && d.sample_amplitude) {
            if (a.nt > 0) return fail(ctx, "diffuse components must precede the global-amplitude ones in a CG group");
            if (a.ng >= MAXG) return fail(ctx, "too many components in CG group");
            a.gc[a.ng++] = l;
        } else if ((ctx->plane_nz[l] & planes) || d.type == DANGX_TCMB || is_global_type(d.type)) {
            a.oc[a.no++] = l;  // (all-zero plane: 0*sed, skipped)
        }
    }
    if (a.ng + a.nt == 0) return fail(ctx, "Woah there, number of CG components = 0 for CG group " + std::to_string(group));
    return 0;
}

// sum of block partials -> host double (deterministic order)
int reduce_to_host(dangx_ctx* ctx, long long nblk, double* out) {
    {
        Timed t(ctx, DANGX_K_REDUCE);
        hipLaunchKernelGGL(k_reduce, dim3(1), dim3(BLOCK), 0, ctx->stream, ctx->partial, nblk, ctx->scalars);
    }
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->scalars, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
// sums of `rows` rows of block partials ([rows][nblk] in ctx->partial) -> host doubles, one block per row (deterministic order)
int rows_to_host(dangx_ctx* ctx, long long nblk, int rows, double* out) {
    hipLaunchKernelGGL(k_reduce_rows_final, dim3(rows), dim3(BLOCK), 0, ctx->stream, ctx->partial, nblk, rows, ctx->rows_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->rows_out, sizeof(double) * rows, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// sum of host doubles over the ranks of a pixel-sharded run (dangx_set_allreduce); identity on a single rank
int rank_sum(dangx_ctx* ctx, double* buf, int64_t n) {
    if (!ctx->allreduce || n <= 0) return 0;
    if (ctx->allreduce(ctx->allreduce_user, buf, n)) return fail(ctx, "the all-reduce callback reported an error");
    return 0;
}
// host <-> device copy of `planes` maps of this shard.  The host side is either a packed [planes][npix] array or, after
// dangx_set_host_stride, a window into full-sky arrays: plane q starts host_stride doubles after plane q-1.
int copy_planes(dangx_ctx* ctx, void* dst, const void* src, size_t planes, bool to_device) {
    const size_t row = (size_t)ctx->dims.npix * sizeof(double);
    const size_t hs = (size_t)(ctx->host_stride > 0 ? ctx->host_stride : ctx->dims.npix) * sizeof(double);
    if (hs == row) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, row * planes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
    } else if (to_device) {
        HIPCHK(ctx, hipMemcpy2DAsync(dst, row, src, hs, row, planes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        HIPCHK(ctx, hipMemcpy2DAsync(dst, hs, src, row, row, planes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
// element (plane q, pixel t) of a host map array under the current host layout
inline double host_at(const dangx_ctx* ctx, const double* a, long long q, long long t) {
    return a[q * (ctx->host_stride > 0 ? ctx->host_stride : ctx->dims.npix) + t];
}
// whether pred holds for every pixel t >= from of plane q of a host map array (stops at the first that fails)
template <class P>
static bool plane_all(const dangx_ctx* ctx, const double* a, long long q, P&& pred, long long from = 0) {
    for (long long t = from; t < ctx->dims.npix; ++t)
        if (!pred(host_at(ctx, a, q, t))) return false;
    return true;
}
// bit k: pred holds for every pixel of plane k of a host [nmaps][npix] array
template <class P>
static unsigned planes_where(const dangx_ctx* ctx, const double* a, P&& pred) {
    unsigned bits = 0;
    for (int k = 0; k < ctx->dims.nmaps; ++k)
        if (plane_all(ctx, a, k, pred)) bits |= 1u << k;
    return bits;
}
// ... and the planes that hold a non-zero value: those that are not zero everywhere
static unsigned planes_nonzero(const dangx_ctx* ctx, const double* a) {
    return ((1u << ctx->dims.nmaps) - 1u) & ~planes_where(ctx, a, [](double v) { return !(v != 0.0); });
}

int check_comp(dangx_ctx* ctx, int comp) {
    if (comp < 0 || comp >= ctx->dims.ncomp) return fail(ctx, "component index out of range");
    return 0;
}

// c%amplitude / c%indices of a component, zero-initialised, unless the caller's device buffers were adopted
int ensure_state(dangx_ctx* ctx, int comp) {
    if (!ctx->comp_set[comp]) return fail(ctx, "component not set");
    (void)hipSetDevice(ctx->device);
    const size_t plane = (size_t)ctx->dims.npix * ctx->dims.nmaps * sizeof(double);
    if (!ctx->amp[comp]) {
        HIPCHK(ctx, hipMalloc(&ctx->amp[comp], plane));
        HIPCHK(ctx, hipMemset(ctx->amp[comp], 0, plane));
        ctx->own_amp[comp] = true; ctx->dirty = true;
    }
    const int nind = ctx->desc[comp].nindices;
    if (nind > 0 && !ctx->idx[comp]) {
        HIPCHK(ctx, hipMalloc(&ctx->idx[comp], plane * nind));
        HIPCHK(ctx, hipMemset(ctx->idx[comp], 0, plane * nind));
        ctx->own_idx[comp] = true; ctx->dirty = true;
        ctx->qu_equal[comp] = (1u << nind) - 1u;
        idx_written(ctx, comp);
    }
    return 0;
}

// ======================================================================= C ABI

extern "C" {

const char* dangx_version(void) { return "dangx 0.1 (gfx950)"; }

int dangx_create(dangx_ctx** out, const dangx_dims* dims) {
    if (!out || !dims) return 1;
    *out = nullptr;
    if (dims->npix <= 0 || (dims->nmaps != 1 && dims->nmaps != 3) || dims->nbands <= 0 || dims->nbands > MAXB ||
        dims->ncomp <= 0 || dims->ncomp > MAXC)
        return 2;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return 3;  // no HIP device: fail loudly, no CPU fallback
    dangx_ctx* ctx = new dangx_ctx();
    ctx->dims = *dims;
    if (dims->device >= 0) {
        if (hipSetDevice(dims->device) != hipSuccess) { delete ctx; return 4; }
        ctx->device = dims->device;
    } else {
        (void)hipGetDevice(&ctx->device);
    }
    Model& M = ctx->hm;
    std::memset(&M, 0, sizeof(M));
    M.npix = dims->npix; M.nmaps = dims->nmaps; M.nbands = dims->nbands; M.ncomp = dims->ncomp;
    M.pix0 = dims->pix0; M.tcmb = 2.7255;  // src/dang_util_mod.f90:15
    for (int j = 0; j < MAXB; ++j) { M.gain[j] = 1.0; M.offset[j] = 0.0; }  // src/dang_data_mod.f90:127-128
    if (hipMalloc(&ctx->dm, sizeof(Model)) != hipSuccess || hipMalloc(&ctx->scalars, 8 * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->chi_cache, CHI_CACHE_DOUBLES * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->chi_stage, sizeof(double) * dangx_ctx::CHI_RING * CHI_ROWS * CHI_RSTAGE) != hipSuccess ||
        hipMalloc(&ctx->rows_out, (4 * MAXB + 8) * sizeof(double)) != hipSuccess ||
        hipMalloc(&ctx->counters, 16 * sizeof(unsigned long long)) != hipSuccess) {
        delete ctx;
        return 5;
    }
    *out = ctx;
    return 0;
}

int dangx_destroy(dangx_ctx* ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    dx_moments_free(ctx);
    if (ctx->own_data) { (void)hipFree(ctx->sig); (void)hipFree(ctx->rms); (void)hipFree(ctx->mask); }
    for (int l = 0; l < MAXC; ++l) {
        if (ctx->amp[l] && ctx->own_amp[l]) (void)hipFree(ctx->amp[l]);
        if (ctx->idx[l] && ctx->own_idx[l]) (void)hipFree(ctx->idx[l]);
    }
    for (auto& w : ctx->work) if (w) (void)hipFree(w);
    if (ctx->partial) (void)hipFree(ctx->partial);
    for (int l = 0; l < MAXC; ++l) if (ctx->tmpl[l]) (void)hipFree(ctx->tmpl[l]);
    if (ctx->d_bp_nu0) { (void)hipFree(ctx->d_bp_nu0); (void)hipFree(ctx->d_bp_tau0); (void)hipFree(ctx->d_bp_lnr); }
    if (ctx->fs_data) (void)hipFree(ctx->fs_data);
    // HEALPix index tables and the degraded maps of the coarse-Nside sweeps live as long as the context
    for (int** b : {&ctx->hp_n2r_f, &ctx->hp_r2n_f, &ctx->hp_n2r_c, &ctx->hp_r2n_c}) { if (*b) (void)hipFree(*b); *b = nullptr; }
    for (double** b : {&ctx->cs_data, &ctx->cs_rms, &ctx->cs_mask, &ctx->cs_index}) { if (*b) (void)hipFree(*b); *b = nullptr; }
    for (auto& kq : ctx->cs_kept) { if (kq.rms) (void)hipFree(kq.rms); if (kq.mask) (void)hipFree(kq.mask); kq.rms = kq.mask = nullptr; kq.cap = kq.capm = 0; kq.gen = -1; }
    if (ctx->cs_part) (void)hipFree(ctx->cs_part);
    ctx->cs_part = nullptr; ctx->cs_part_cap = 0;
    for (double** b : {&ctx->cs_model, &ctx->cm_part}) { if (*b) (void)hipFree(*b); *b = nullptr; }
    ctx->cm_cap = ctx->cm_part_cap = 0;
    ctx->hp_nside = ctx->hp_cnside = 0; ctx->cs_cap = 0;
    (void)hipFree(ctx->rows_out);
    (void)hipFree(ctx->dm); (void)hipFree(ctx->scalars); (void)hipFree(ctx->counters); (void)hipFree(ctx->chi_cache);
    for (auto& p : ctx->chi_pend) if (p.buf) (void)hipFree(p.buf);
    if (ctx->chi_stage) (void)hipFree(ctx->chi_stage);
    for (auto& e : ctx->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    dx_rtc_release(ctx);
    delete ctx;
    return 0;
}

const char* dangx_last_error(const dangx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dangx_set_stream(dangx_ctx* ctx, void* s) {
    if (!ctx) return 1;
    if ((hipStream_t)s != ctx->stream) {
        // chi^2 block partials of the sweeps launched so far wait in the ring: reduce them on the stream that produced
        // them, and let everything enqueued there finish before the first launch on the new stream can overtake it
        (void)hipSetDevice(ctx->device);
        if (chi_flush(ctx)) return 1;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->stream = (hipStream_t)s;
    return 0;
}

int dangx_set_allreduce(dangx_ctx* ctx, dangx_allreduce_fn fn, void* user, int is_root) {
    if (!ctx) return 1;
    ctx->allreduce = fn; ctx->allreduce_user = user; ctx->is_root = (fn == nullptr) || is_root != 0;
    return 0;
}

int dangx_device_count(int* n) {
    if (!n) return 1;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return 0;
}

int dangx_set_host_stride(dangx_ctx* ctx, int64_t plane_stride) {
    if (!ctx) return 1;
    if (plane_stride != 0 && plane_stride < ctx->dims.npix) return fail(ctx, "host plane stride smaller than the shard");
    ctx->host_stride = plane_stride;
    return 0;
}

int dangx_synchronize(dangx_ctx* ctx) {
    if (!ctx) return 1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_set_band(dangx_ctx* ctx, int band, double nu_c, int n, const double* nu0, const double* tau0) {
    if (!ctx) return 1;
    if (band < 0 || band >= ctx->dims.nbands) return fail(ctx, "band index out of range");
    if (n < 0 || (n > 0 && (!nu0 || !tau0))) return fail(ctx, "bad bandpass arrays");
    Band& b = ctx->hm.band[band];
    b.nu_c = (nu_c < 1e9) ? nu_c * 1e9 : nu_c;  // src/dang_bp_mod.f90:35-37
    b.n = n;
    b.off = (int)ctx->bp_nu0.size();
    for (int i = 0; i < n; ++i) { ctx->bp_nu0.push_back(nu0[i]); ctx->bp_tau0.push_back(tau0[i]); }
    ctx->band_set[band] = true;
    ctx->dirty = true; ctx->bp_dirty = true;
    invalidate_chi(ctx);
    return 0;
}

int dangx_set_component(dangx_ctx* ctx, int comp, const dangx_comp_desc* d) {
    if (!ctx || !d) return 1;
    if (check_comp(ctx, comp)) return 1;
    if (d->type < DANGX_POWERLAW || d->type > DANGX_HIFIT)
        return fail(ctx, "Error - unrecognized component type (only diffuse types are built)");
    const int want = (d->type == DANGX_MBB || d->type == DANGX_LOGNORMAL) ? 2
                     : (d->type == DANGX_CMB || d->type == DANGX_TEMPLATE || d->type == DANGX_MONOPOLE) ? 0 : 1;
    if (d->nindices != want) return fail(ctx, "nindices does not match the component type");
    // the amplitude / index maps are allocated on first use (ensure_state): a caller that adopts its own device
    // buffers (dangx_adopt_device_state) never holds two copies
    ctx->desc[comp] = *d;
    if (ctx->desc[comp].nu_ref < 1e7) ctx->desc[comp].nu_ref *= 1e9;  // src/dang_param_mod.f90:571-573
    ctx->comp_set[comp] = true;
    ctx->dirty = true; ctx->bp_dirty = true;
    invalidate_chi(ctx);
    return 0;
}

int dangx_set_tcmb(dangx_ctx* ctx, double T) {
    if (!ctx) return 1;
    ctx->hm.tcmb = T;
    ctx->dirty = true;
    invalidate_chi(ctx);
    return 0;
}

int dangx_set_calibration(dangx_ctx* ctx, const double* gain, const double* offset) {
    if (!ctx) return 1;
    for (int j = 0; j < ctx->dims.nbands; ++j) {
        if (gain) ctx->hm.gain[j] = gain[j];
        if (offset) ctx->hm.offset[j] = offset[j];
    }
    ctx->dirty = true;
    invalidate_chi(ctx);
    return 0;
}

int dangx_upload_data(dangx_ctx* ctx, const double* sig, const double* rms, const double* mask) {
    if (!ctx || !sig || !rms || !mask) return 1;
    (void)hipSetDevice(ctx->device);
    const size_t nmap = (size_t)ctx->dims.npix * ctx->dims.nmaps * sizeof(double);
    const size_t nall = nmap * ctx->dims.nbands;
    if (!ctx->own_data) {
        ctx->sig = ctx->rms = ctx->mask = nullptr;
        HIPCHK(ctx, hipMalloc(&ctx->sig, nall));
        HIPCHK(ctx, hipMalloc(&ctx->rms, nall));
        HIPCHK(ctx, hipMalloc(&ctx->mask, nmap));
        ctx->own_data = true;
    }
    const size_t nplanes = (size_t)ctx->dims.nmaps * ctx->dims.nbands;
    if (copy_planes(ctx, ctx->sig, sig, nplanes, true) || copy_planes(ctx, ctx->rms, rms, nplanes, true) ||
        copy_planes(ctx, ctx->mask, mask, (size_t)ctx->dims.nmaps, true))
        return 1;
    ctx->dirty = true;
    ++ctx->data_gen;
    invalidate_chi(ctx);
    idx_written(ctx, -1);   // a new mask
    return 0;
}

int dangx_adopt_device_data(dangx_ctx* ctx, const double* sig, const double* rms, const double* mask) {
    if (!ctx || !sig || !rms || !mask) return 1;
    if (ctx->own_data) { (void)hipFree(ctx->sig); (void)hipFree(ctx->rms); (void)hipFree(ctx->mask); ctx->own_data = false; }
    ctx->sig = const_cast<double*>(sig);
    ctx->rms = const_cast<double*>(rms);
    ctx->mask = const_cast<double*>(mask);
    ctx->dirty = true;
    ++ctx->data_gen;
    invalidate_chi(ctx);
    idx_written(ctx, -1);
    return 0;
}

int dangx_put_amplitude(dangx_ctx* ctx, int comp, const double* amp) {
    if (!ctx || !amp || check_comp(ctx, comp) || ensure_state(ctx, comp)) return 1;
    invalidate_chi(ctx);
    ctx->plane_nz[comp] = planes_nonzero(ctx, amp);
    return copy_planes(ctx, ctx->amp[comp], amp, (size_t)ctx->dims.nmaps, true);
}
int dangx_get_amplitude(dangx_ctx* ctx, int comp, double* amp) {
    if (!ctx || !amp || check_comp(ctx, comp) || ensure_state(ctx, comp)) return 1;
    return copy_planes(ctx, amp, ctx->amp[comp], (size_t)ctx->dims.nmaps, false);
}
int dangx_put_indices(dangx_ctx* ctx, int comp, const double* ind) {
    if (!ctx || !ind || check_comp(ctx, comp) || ensure_state(ctx, comp)) return 1;
    if (!ctx->idx[comp]) return fail(ctx, "component has no indices");
    invalidate_chi(ctx);
    idx_written(ctx, comp);
    {   // planes on which every index map is spatially constant
        const long long np = ctx->dims.npix;
        ctx->idx_const[comp] = 0;
        for (int k = 0; k < ctx->dims.nmaps; ++k) {
            bool cst = true;
            for (int q = 0; q < ctx->desc[comp].nindices && cst; ++q) {
                const long long pl = (long long)q * ctx->dims.nmaps + k;
                const double m0 = host_at(ctx, ind, pl, 0);
                cst = plane_all(ctx, ind, pl, [m0](double v) { return !(v != m0); }, 1);
                ctx->idx_val[comp][k][q] = m0;
            }
            if (cst) ctx->idx_const[comp] |= 1u << k;
        }
        ctx->qu_equal[comp] = 0;
        for (int q = 0; q < ctx->desc[comp].nindices && ctx->dims.nmaps == 3; ++q) {
            bool eq = true;
            for (long long t = 0; t < np && eq; ++t) eq = host_at(ctx, ind, (long long)q * 3 + 1, t) == host_at(ctx, ind, (long long)q * 3 + 2, t);
            if (eq) ctx->qu_equal[comp] |= 1u << q;
        }
        ctx->dirty = true;
    }
    return copy_planes(ctx, ctx->idx[comp], ind, (size_t)ctx->dims.nmaps * ctx->desc[comp].nindices, true);
}
int dangx_get_indices(dangx_ctx* ctx, int comp, double* ind) {
    if (!ctx || !ind || check_comp(ctx, comp) || ensure_state(ctx, comp)) return 1;
    if (!ctx->idx[comp]) return fail(ctx, "component has no indices");
    return copy_planes(ctx, ind, ctx->idx[comp], (size_t)ctx->dims.nmaps * ctx->desc[comp].nindices, false);
}
int dangx_set_template(dangx_ctx* ctx, int comp, const double* tmpl, const int32_t* corr, int nfit) {
    if (!ctx || !tmpl || !corr || check_comp(ctx, comp)) return 1;
    if (!ctx->comp_set[comp] || !is_global_type(ctx->desc[comp].type)) return fail(ctx, "not a template / monopole / hi_fit component");
    (void)hipSetDevice(ctx->device);
    int mask = 0, cnt = 0;
    for (int j = 0; j < ctx->dims.nbands; ++j) if (corr[j]) { mask |= 1 << j; ++cnt; }
    if (cnt != nfit) return fail(ctx, "nfit does not match the number of fitted (corr) bands");
    const size_t bytes = (size_t)ctx->dims.npix * ctx->dims.nmaps * sizeof(double);
    if (!ctx->tmpl[comp]) HIPCHK(ctx, hipMalloc(&ctx->tmpl[comp], bytes));
    if (copy_planes(ctx, ctx->tmpl[comp], tmpl, (size_t)ctx->dims.nmaps, true)) return 1;
    ctx->tmpl_nz[comp] = planes_nonzero(ctx, tmpl);   // planes on which the template is identically zero carry none of its signal (a Q/U template on T)
    ctx->tmpl_one[comp] = planes_where(ctx, tmpl, [](double v) { return v == 1.0; });
    ctx->corr_mask[comp] = mask; ctx->nfit[comp] = nfit;
    ctx->dirty = true;
    invalidate_chi(ctx);
    return 0;
}
int dangx_put_template_amplitudes(dangx_ctx* ctx, int comp, const double* ta) {
    if (!ctx || !ta || check_comp(ctx, comp)) return 1;
    for (int k = 0; k < ctx->dims.nmaps; ++k)
        for (int j = 0; j < ctx->dims.nbands; ++j) ctx->tamp[comp][k][j] = ta[k * ctx->dims.nbands + j];
    if (ctx->desc[comp].type == DANGX_MONOPOLE)
        for (int j = 0; j < ctx->dims.nbands; ++j) ctx->hm.offset[j] = ctx->tamp[comp][0][j];
    ctx->dirty = true;
    invalidate_chi(ctx);
    return 0;
}
int dangx_get_template_amplitudes(dangx_ctx* ctx, int comp, double* ta) {
    if (!ctx || !ta || check_comp(ctx, comp)) return 1;
    for (int k = 0; k < ctx->dims.nmaps; ++k)
        for (int j = 0; j < ctx->dims.nbands; ++j) ta[k * ctx->dims.nbands + j] = ctx->tamp[comp][k][j];
    return 0;
}

int dangx_adopt_device_state(dangx_ctx* ctx, int comp, double* amp_dev, double* idx_dev) {
    if (!ctx || !amp_dev || check_comp(ctx, comp)) return 1;
    if (!ctx->comp_set[comp]) return fail(ctx, "component not set");
    if (ctx->desc[comp].nindices > 0 && !idx_dev) return fail(ctx, "component has indices: idx_dev required");
    if (ctx->amp[comp] && ctx->own_amp[comp]) (void)hipFree(ctx->amp[comp]);
    if (ctx->idx[comp] && ctx->own_idx[comp]) (void)hipFree(ctx->idx[comp]);
    invalidate_chi(ctx);
    ctx->amp[comp] = amp_dev; ctx->own_amp[comp] = false;
    {   // which planes hold a non-zero amplitude right now (one small kernel, once)
        unsigned f = 0;
        unsigned* df = reinterpret_cast<unsigned*>(ctx->counters + 2);
        HIPCHK(ctx, hipMemsetAsync(df, 0, sizeof(unsigned), ctx->stream));
        hipLaunchKernelGGL(k_any_nonzero, dim3(1024), dim3(BLOCK), 0, ctx->stream, amp_dev, (long long)ctx->dims.npix, ctx->dims.nmaps, df);
        HIPCHK(ctx, hipMemcpyAsync(&f, df, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->plane_nz[comp] = f;
    }
    ctx->idx[comp] = (ctx->desc[comp].nindices > 0) ? idx_dev : nullptr; ctx->own_idx[comp] = false;
    ctx->idx_ext[comp] = true;   // the caller may write these maps at any time
    idx_written(ctx, comp);
    ctx->idx_const[comp] = 0;
    if (ctx->idx[comp]) {   // planes on which every index map is spatially constant (one small kernel, once)
        const int nind = ctx->desc[comp].nindices, nmaps = ctx->dims.nmaps;
        unsigned f = 0;
        double first[6] = {};
        unsigned* df = reinterpret_cast<unsigned*>(ctx->counters + 2);
        HIPCHK(ctx, hipMemsetAsync(df, 0, sizeof(unsigned), ctx->stream));
        hipLaunchKernelGGL(k_not_constant, dim3(1024), dim3(BLOCK), 0, ctx->stream, idx_dev, (long long)ctx->dims.npix, nmaps, nind, df, ctx->scalars + 2);
        HIPCHK(ctx, hipMemcpyAsync(&f, df, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(first, ctx->scalars + 2, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < nmaps; ++k) {
            bool cst = true;
            for (int q = 0; q < nind; ++q) {
                if ((f >> (q * 3 + k)) & 1) cst = false;
                ctx->idx_val[comp][k][q] = first[q * 3 + k];
            }
            if (cst) ctx->idx_const[comp] |= 1u << k;
        }
        ctx->qu_equal[comp] = 0;
        if (nmaps == 3) {
            unsigned dq = 0;
            HIPCHK(ctx, hipMemsetAsync(df, 0, sizeof(unsigned), ctx->stream));
            hipLaunchKernelGGL(k_qu_differ, dim3(1024), dim3(BLOCK), 0, ctx->stream, idx_dev, (long long)ctx->dims.npix, nind, df);
            HIPCHK(ctx, hipMemcpyAsync(&dq, df, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            ctx->qu_equal[comp] = ~dq & ((1u << nind) - 1u);
        }
    }
    ctx->dirty = true;
    return 0;
}
void* dangx_amplitude_devptr(dangx_ctx* ctx, int comp) {
    return (ctx && comp >= 0 && comp < ctx->dims.ncomp && !ensure_state(ctx, comp)) ? ctx->amp[comp] : nullptr;
}
void* dangx_indices_devptr(dangx_ctx* ctx, int comp) {
    return (ctx && comp >= 0 && comp < ctx->dims.ncomp && !ensure_state(ctx, comp)) ? ctx->idx[comp] : nullptr;
}

// local (this shard's) sum of c%indices(:, map_n, nind) over unmasked pixels and their number: mask_avg = sum / count
int dangx_index_masked_sum(dangx_ctx* ctx, int comp, int nind, int map_n, double* sum, int64_t* count) {
    if (!ctx || !sum || !count || check_comp(ctx, comp)) return 1;
    (void)hipSetDevice(ctx->device);
    if (nind < 0 || nind >= ctx->desc[comp].nindices) return fail(ctx, "index number out of range");
    if (map_n < 1 || map_n > ctx->dims.nmaps) return fail(ctx, "map_n must be a map number (1..nmaps)");
    if (sync_model(ctx)) return 1;
    const unsigned nblk = nblocks(ctx->hm.npix);
    if (ensure_partial(ctx, 2ll * nblk)) return 1;
    hipLaunchKernelGGL(k_index_masked_sum, dim3(nblk), dim3(BLOCK), 0, ctx->stream, ctx->dm, comp, nind, map_n, ctx->partial);
    double out[2] = {0.0, 0.0};
    if (rows_to_host(ctx, nblk, 2, out)) return 1;
    *sum = out[0];
    *count = (int64_t)out[1];
    return 0;
}

// the masked sums of up to 16 index maps in ONE launch and ONE wait (write_stats_to_term prints them all after every phase,
// src/dang_data_mod.f90:540-567; write_data every iteration, :716-731)
int dangx_index_masked_sums(dangx_ctx* ctx, int n, const int32_t* comp, const int32_t* nind, const int32_t* map_n, double* sums, int64_t* counts) {
    if (!ctx || n < 1 || n > 16 || !comp || !nind || !map_n || !sums || !counts) return 1;
    (void)hipSetDevice(ctx->device);
    MeanList ml;
    ml.n = n;
    for (int e = 0; e < 16; ++e) { ml.comp[e] = 0; ml.nind[e] = 0; ml.k[e] = 1; }
    for (int e = 0; e < n; ++e) {
        if (check_comp(ctx, comp[e])) return 1;
        if (nind[e] < 0 || nind[e] >= ctx->desc[comp[e]].nindices) return fail(ctx, "index number out of range");
        if (map_n[e] < 1 || map_n[e] > ctx->dims.nmaps) return fail(ctx, "map_n must be a map number (1..nmaps)");
        ml.comp[e] = comp[e]; ml.nind[e] = nind[e]; ml.k[e] = map_n[e];
    }
    // what is still valid from an earlier call (nothing has written these maps or the mask since) is answered from the host:
    // the statistics after an amplitude phase (src/dang_cg_mod.f90:173) repeat the index means of the phase before; what the
    // last plane-set launch left on the device beside its chi^2 sums (the sums of the maps it swept) costs one small copy
    bool all_known = true, need_copy = false;
    for (int e = 0; e < n; ++e) {
        const int l = comp[e], q = nind[e], k = map_n[e] - 1;
        if (ctx->idx_ext[l] || (!ctx->idxsum_ok[l][q][k] && !(ctx->idxsum_dev[l][q][k] && ctx->mask_count >= 0))) all_known = false;
        else if (!ctx->idxsum_ok[l][q][k]) need_copy = true;
    }
    if (all_known && need_copy) {
        if (chi_flush(ctx)) return 1;
        double host[CHI_CACHE_DOUBLES];
        HIPCHK(ctx, hipMemcpyAsync(host, ctx->chi_cache, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int l = 0; l < ctx->hm.ncomp; ++l)
            for (int q = 0; q < MAXI; ++q)
                for (int k = 0; k < 3; ++k)
                    if (ctx->idxsum_dev[l][q][k] && !ctx->idxsum_ok[l][q][k]) {
                        ctx->idxsum[l][q][k] = host[idx_slot(l, q, k + 1)];
                        ctx->idxcnt[l][q][k] = ctx->mask_count;
                        ctx->idxsum_ok[l][q][k] = true;
                    }
    }
    if (all_known) {
        for (int e = 0; e < n; ++e) { sums[e] = ctx->idxsum[comp[e]][nind[e]][map_n[e] - 1]; counts[e] = ctx->idxcnt[comp[e]][nind[e]][map_n[e] - 1]; }
        return 0;
    }
    if (sync_model(ctx)) return 1;
    const unsigned nblk = std::min(nblocks(ctx->hm.npix), 4096u);
    if (ensure_partial(ctx, 2ll * n * nblk)) return 1;
    if (ensure_work(ctx, 64)) return 1;
    hipLaunchKernelGGL(k_index_masked_sums, dim3(nblk), dim3(BLOCK), 0, ctx->stream, ctx->dm, ml, ctx->partial);
    hipLaunchKernelGGL(k_reduce_rows_final, dim3(2 * n), dim3(BLOCK), 0, ctx->stream, ctx->partial, (long long)nblk, 2 * n, ctx->work[0]);
    HIPCHK(ctx, hipGetLastError());
    double out[32];
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->work[0], sizeof(double) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int e = 0; e < n; ++e) {
        sums[e] = out[2 * e]; counts[e] = (int64_t)out[2 * e + 1];
        ctx->idxsum[comp[e]][nind[e]][map_n[e] - 1] = sums[e]; ctx->idxcnt[comp[e]][nind[e]][map_n[e] - 1] = counts[e];
        ctx->idxsum_ok[comp[e]][nind[e]][map_n[e] - 1] = !ctx->idx_ext[comp[e]];
    }
    ctx->mask_count = counts[0];   // unmasked pixels of masks(:,1): the same for every map
    return 0;
}

// local sums over every pixel of c%indices(:, map_n, nind) and of masks(:,1) (see k_index_plain_sum)
int dangx_index_plain_sum(dangx_ctx* ctx, int comp, int nind, int map_n, double* sum_index, double* sum_mask) {
    if (!ctx || !sum_index || !sum_mask || check_comp(ctx, comp)) return 1;
    (void)hipSetDevice(ctx->device);
    if (nind < 0 || nind >= ctx->desc[comp].nindices) return fail(ctx, "index number out of range");
    if (map_n < 1 || map_n > ctx->dims.nmaps) return fail(ctx, "map_n must be a map number (1..nmaps)");
    if (sync_model(ctx)) return 1;
    const unsigned nblk = nblocks(ctx->hm.npix);
    if (ensure_partial(ctx, 2ll * nblk)) return 1;
    hipLaunchKernelGGL(k_index_plain_sum, dim3(nblk), dim3(BLOCK), 0, ctx->stream, ctx->dm, comp, nind, map_n, ctx->partial);
    double out[2] = {0.0, 0.0};
    if (rows_to_host(ctx, nblk, 2, out)) return 1;
    *sum_index = out[0];
    *sum_mask = out[1];
    return 0;
}

int dangx_unit_conversion(dangx_ctx* ctx, int band, int which, double* out) {
    if (!ctx || !out) return 1;
    if (band < 0 || band >= ctx->dims.nbands || !ctx->band_set[band]) return fail(ctx, "band index out of range / band not set");
    switch (which) {
    case DANGX_A2T: *out = host_a2t(ctx, band); return 0;
    case DANGX_A2F: *out = host_a2f(ctx, band); return 0;
    case DANGX_F2T: *out = host_f2t(ctx, band); return 0;
    default: return fail(ctx, "unit conversion selector must be DANGX_A2T, DANGX_A2F or DANGX_F2T");
    }
}

int dangx_normalize_bandpass(const double* tau_in, int n, double* tau_out) {
    if (!tau_in || !tau_out || n <= 0) return 1;
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += tau_in[i];   // total = sum(tau_in)
    for (int i = 0; i < n; ++i) tau_out[i] = tau_in[i] / total;
    return 0;
}

int dangx_convert_maps(dangx_ctx* ctx, const int32_t* unit, const int32_t* cg_map, double* conversion) {
    if (ctx) ++ctx->data_gen;   // the maps are rescaled in place
    if (!ctx || !unit || !conversion) return 1;
    (void)hipSetDevice(ctx->device);
    if (!ctx->sig || !ctx->rms) return fail(ctx, "map data not uploaded");
    const int nb = ctx->dims.nbands;
    for (int j = 0; j < nb; ++j)
        if (!ctx->band_set[j]) return fail(ctx, "band " + std::to_string(j) + " not set");
    const long long plane = (long long)ctx->dims.nmaps * ctx->dims.npix;
    for (int j = 0; j < nb; ++j) {
        if (cg_map && cg_map[j]) continue;  // :435 `if (.not. self%cg_map(j))`: swapped-in maps are converted by convert_cg_maps
        double f;
        if (unit[j] == DANGX_UNIT_UK_RJ) f = 1.0;
        else if (unit[j] == DANGX_UNIT_UK_CMB) f = 1.0 / host_a2t(ctx, j);
        else if (unit[j] == DANGX_UNIT_MJY_SR) f = 1.0 / host_a2f(ctx, j);
        else return fail(ctx, "Not a unit, dumbass! (unit code " + std::to_string(unit[j]) + ")");
        conversion[j] = f;
        hipLaunchKernelGGL(k_scale_band, dim3(nblocks(plane)), dim3(BLOCK), 0, ctx->stream, const_cast<double*>(ctx->sig) + (long long)j * plane,
                           const_cast<double*>(ctx->rms) + (long long)j * plane, plane, f);
        ctx->hm.offset[j] = ctx->hm.offset[j] * f;
        // "Set the loaded monopole values into the monopole component" (:453-457): after EVERY converted band the whole
        // offset vector goes into template_amplitudes(:,1) of every monopole
        for (int l = 0; l < ctx->dims.ncomp; ++l)
            if (ctx->comp_set[l] && ctx->desc[l].type == DANGX_MONOPOLE)
                for (int jj = 0; jj < nb; ++jj) ctx->tamp[l][0][jj] = ctx->hm.offset[jj];
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->dirty = true;
    invalidate_chi(ctx);
    return 0;
}

int dangx_fill_index(dangx_ctx* ctx, int comp, int nind, int map_n, double value) {
    if (!ctx || check_comp(ctx, comp)) return 1;
    (void)hipSetDevice(ctx->device);
    int s1, s2;
    if (map_planes(ctx, map_n, s1, s2)) return 1;
    if (nind < 0 || nind >= ctx->desc[comp].nindices) return fail(ctx, "index number out of range");
    if (sync_model(ctx)) return 1;
    hipLaunchKernelGGL(k_fill_index, dim3(nblocks(ctx->hm.npix)), dim3(BLOCK), 0, ctx->stream, ctx->dm, comp, nind, s1, s2, value);
    HIPCHK(ctx, hipGetLastError());
    // the map is spatially constant on those planes now iff the component's other indices are; re-derive lazily:
    // simply mark the planes non-constant unless the component has a single index
    for (int k = s1; k <= s2; ++k) {
        if (ctx->desc[comp].nindices == 1) { ctx->idx_const[comp] |= 1u << (k - 1); ctx->idx_val[comp][k - 1][0] = value; }
        else if (ctx->idx_const[comp] & (1u << (k - 1))) ctx->idx_val[comp][k - 1][nind] = value;
        ctx->chi_before_valid[k - 1] = ctx->chi_after_valid[k - 1] = false;
    }
    idx_written(ctx, comp);
    qu_written(ctx, comp, nind, map_n);
    ctx->dirty = true;
    return 0;
}

// c%indices(pix, map_n, 0:nindices-1) of one (local) pixel -> out[nindices]
int dangx_peek_indices(dangx_ctx* ctx, int comp, int map_n, long long pix, double* out) {
    if (!ctx || !out || check_comp(ctx, comp)) return 1;
    if (!ctx->idx[comp]) return fail(ctx, "component has no indices");
    if (map_n < 1 || map_n > ctx->dims.nmaps || pix < 0 || pix >= ctx->dims.npix) return fail(ctx, "bad map/pixel");
    for (int q = 0; q < ctx->desc[comp].nindices; ++q)
        HIPCHK(ctx, hipMemcpyAsync(out + q, ctx->idx[comp] + ((long long)q * ctx->dims.nmaps + (map_n - 1)) * ctx->dims.npix + pix,
                                   sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// fit_band_gain sums for band (0-based), map_n = 1: out[0] = sum map2*N_inv*map1, out[1] = sum map1*N_inv*map1
int dangx_gain_sums(dangx_ctx* ctx, int band, double* out) {
    if (!ctx || !out) return 1;
    (void)hipSetDevice(ctx->device);
    if (band < 0 || band >= ctx->dims.nbands) return fail(ctx, "band index out of range");
    if (sync_model(ctx)) return 1;
    const unsigned nblk = nblocks(ctx->hm.npix);
    if (ensure_partial(ctx, 2ll * nblk)) return 1;
    hipLaunchKernelGGL(k_gain_rows, dim3(nblk), dim3(BLOCK), 0, ctx->stream, ctx->dm, band, ctx->partial);
    return rows_to_host(ctx, nblk, 2, out);
}

// ---- profiling ---------------------------------------------------------------------

int dangx_profile_enable(dangx_ctx* ctx, int on) {
    if (!ctx) return 1;
    ctx->prof = on != 0;
    return 0;
}
int dangx_profile_reset(dangx_ctx* ctx) {
    if (!ctx) return 1;
    if (prof_collect(ctx)) return 1;
    for (int k = 0; k < DANGX_K_COUNT; ++k) {
        ctx->prof_ms[k] = 0.0; ctx->prof_n[k] = 0;
        for (int p = 0; p < 3; ++p) { ctx->prof_ms_pl[k][p] = 0.0; ctx->prof_n_pl[k][p] = 0; }
    }
    return 0;
}
int dangx_profile_get(dangx_ctx* ctx, int kid, double* total_ms, int64_t* launches) {
    if (!ctx || kid < 0 || kid >= DANGX_K_COUNT) return 1;
    if (prof_collect(ctx)) return 1;
    if (total_ms) *total_ms = ctx->prof_ms[kid];
    if (launches) *launches = ctx->prof_n[kid];
    return 0;
}
int dangx_profile_get_planes(dangx_ctx* ctx, int kid, int nplanes, double* total_ms, int64_t* launches) {
    if (!ctx || kid < 0 || kid >= DANGX_K_COUNT || nplanes < 1 || nplanes > 2) return 1;
    if (prof_collect(ctx)) return 1;
    if (total_ms) *total_ms = ctx->prof_ms_pl[kid][nplanes];
    if (launches) *launches = ctx->prof_n_pl[kid][nplanes];
    return 0;
}

}  // extern "C"
