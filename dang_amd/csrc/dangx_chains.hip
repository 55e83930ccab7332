// dangx_chains.hip -- dangx_chains_*: read-outs over the accumulators of SEVERAL chains of one device (definitions in dx_chains_host.h).  Nothing here
// touches an accumulator, a chain or a cache: six read-only kernels combine the per-chain planes and write only the map asked for.
//   k_chains_batches  the batched accumulators (dx_batches_host.h): every chain's slots in one pass from one base pointer per chain.
//   k_chains_stat  planes and signals (blockIdx.y = plane, up to three): pooled mean / std, R-hat, W, B/n read K x (mean, m2) --
//                  a stat that does not use one of the two does not load it -- and write one f64: at most (2 K + 1) x 8 B per
//                  element; the pooled ESS reads K x (mean, m2, prev, first, P), (5 K + 1) x 8 B.
//   k_chains_pair  one pair: K x (mean_a, mean_b, C) for the covariance, + K x (m2_a, m2_b) for the correlation.
//   k_chains_angle one polarisation angle (dx_angle_host.h): K x (Cbar, Sbar) pooled by the sample counts and read as one chain's, or
//                  the circular std of the K mean directions; (2 K + 1) x 8 B per element.
//   k_chains_hist  a lane sums its pixel's K records piece by piece in 64-bit integers and takes k_hist_stat's steps on the sums.
//   k_chains_rank  the rank-normalised / folded R-hat of the binned traces (dx_rank_host.h): a lane walks its pixel's K records for
//                  the pooled total, once more for the scores and the K running (n, mean, m2), and for the fold a third time by
//                  32-bit word around the pooled median bin; it writes one f64.
// The pointers of all chains travel by value (ChainsArgs + DxChainsPar: 1.3 KB of the 4 KB kernel-argument segment).  Pairs of elements are read
// as 16 bytes where every pointer of a plane shares out's 16-byte phase, element by element otherwise (chains whose buffers were
// adopted at different alignments; dx_stream.h); both forms evaluate the same header functions.  No LDS, no atomics, no scratch.
// The chains' state is read through DxMoments' accessors (dx_moments_state.h); dangx_moments.hip accumulates it.  A chain may be a
// holder (dangx_moments_begin_like): the accessors then answer from the sections put into it, null for one that was not, which the
// host side refuses by name before a launch.
#include "dx_moments_state.h"
#include "dx_hist_host.h"
#include "dx_chains_host.h"
#include "dx_batches_host.h"
#include "dx_rank_host.h"
#include "dx_stream.h"

static_assert(DX_CHAINS_MAX == DANGX_MAX_CHAINS, "dx_chains_host.h and include/dangx.h disagree");
static_assert(DX_ANG_MAX_CHAINS == DX_CHAINS_MAX, "dx_angle_host.h and dx_chains_host.h disagree");

namespace {

struct ChainsArgs {       // the pointer table of a plane / signal read-out; read through the kernel-argument segment (chains_kptr)
    const double* mean[3][DX_CHAINS_MAX];
    const double* m2[3][DX_CHAINS_MAX];
    const double* prev[3][DX_CHAINS_MAX];    // DX_CH_ESS only
    const double* first[3][DX_CHAINS_MAX];
    const double* P[3][DX_CHAINS_MAX];
    double* out[3];
};
static_assert(sizeof(ChainsArgs) + sizeof(DxChainsPar) <= 2048, "the arguments must stay well inside the 4 KB kernel-argument segment");
// The table is indexed by blockIdx.y: read where the kernel arguments lie (scalar loads at a computed offset), never copied.
// It is the kernels' FIRST argument, i.e. offset 0 of the segment.
typedef const ChainsArgs __attribute__((address_space(4))) * chains_kptr;

// V consecutive elements of plane p from element i on
template <int V>
__device__ __forceinline__ void chains_item(chains_kptr a, const DxChainsPar& par, int stat, int p, long long i) {
    double r[V];
    if (stat == DX_CH_ESS) {
#pragma unroll
        for (int e = 0; e < V; ++e) r[e] = 0.0;
        dx_chains_each<0>(par.K, [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            double m[V], q[V], pv[V], f[V], P[V];
            ChV<V>::ld(a->mean[p][k] + i, m); ChV<V>::ld(a->m2[p][k] + i, q); ChV<V>::ld(a->prev[p][k] + i, pv);
            ChV<V>::ld(a->first[p][k] + i, f); ChV<V>::ld(a->P[p][k] + i, P);
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = dx_chains_ess_add(r[e], m[e], q[e], pv[e], f[e], P[e], par.cnt[k]);
        });
    } else {
        double mean[V][DX_CHAINS_MAX] = {}, m2[V][DX_CHAINS_MAX] = {};
        const bool nm = dx_chains_needs_mean(stat), nq = dx_chains_needs_m2(stat);
        dx_chains_each<0>(par.K, [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            double m[V] = {}, q[V] = {};
            if (nm) ChV<V>::ld(a->mean[p][k] + i, m);
            if (nq) ChV<V>::ld(a->m2[p][k] + i, q);
#pragma unroll
            for (int e = 0; e < V; ++e) { mean[e][k] = m[e]; m2[e][k] = q[e]; }
        });
#pragma unroll
        for (int e = 0; e < V; ++e) r[e] = dx_chains_stat(stat, par, mean[e], m2[e]);
    }
    ChV<V>::st(a->out[p] + i, r);
}

__global__ __launch_bounds__(BLOCK) void k_chains_stat(ChainsArgs, DxChainsPar par, long long n, int stat) {
    const chains_kptr a = (chains_kptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int p = blockIdx.y;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const uintptr_t ao = addr(a->out[p]);
    uintptr_t diff = ao & 7;   // out not even at a double's alignment: element by element
    const bool ess = stat == DX_CH_ESS;
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        diff |= (ao ^ addr(a->mean[p][k])) | (ao ^ addr(a->m2[p][k]));
        if (ess) diff |= (ao ^ addr(a->prev[p][k])) | (ao ^ addr(a->first[p][k])) | (ao ^ addr(a->P[p][k]));
    });
    // dx_stream's loop written out: through dx_stream this kernel compiled to fewer instructions (5618 for 5788) at the same
    // registers and occupancy, but its R-hat and ESS read-outs at Nside 1024 measured 2 % slower than this form, more than the
    // spread of this form's rounds ("Posterior moments on the device")
    if ((diff & 15) != 0) {
        for (long long i = gid; i < n; i += stride) chains_item<1>(a, par, stat, p, i);
        return;
    }
    const long long head = ((ao & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;   // tail < n: one element after the last pair
    if (gid == 0 && head) chains_item<1>(a, par, stat, p, 0);
    if (gid == 1 && tail < n) chains_item<1>(a, par, stat, p, tail);
    for (long long t = gid; t < npair; t += stride) chains_item<2>(a, par, stat, p, head + 2 * t);
}

struct ChainsPairArgs {
    const double* ma[DX_CHAINS_MAX];
    const double* mb[DX_CHAINS_MAX];
    const double* qa[DX_CHAINS_MAX];
    const double* qb[DX_CHAINS_MAX];
    const double* C[DX_CHAINS_MAX];
    double* out;
};

template <int V>
__device__ __forceinline__ void chains_pair_item(const ChainsPairArgs& a, const DxChainsPar& par, int stat, long long i) {
    double ma[V][DX_CHAINS_MAX] = {}, mb[V][DX_CHAINS_MAX] = {}, qa[V][DX_CHAINS_MAX] = {}, qb[V][DX_CHAINS_MAX] = {}, C[V][DX_CHAINS_MAX] = {};
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        double va[V], vb[V], vc[V], wa[V] = {}, wb[V] = {};
        ChV<V>::ld(a.ma[k] + i, va); ChV<V>::ld(a.mb[k] + i, vb); ChV<V>::ld(a.C[k] + i, vc);
        if (stat) { ChV<V>::ld(a.qa[k] + i, wa); ChV<V>::ld(a.qb[k] + i, wb); }
#pragma unroll
        for (int e = 0; e < V; ++e) { ma[e][k] = va[e]; mb[e][k] = vb[e]; qa[e][k] = wa[e]; qb[e][k] = wb[e]; C[e][k] = vc[e]; }
    });
    double r[V];
#pragma unroll
    for (int e = 0; e < V; ++e) r[e] = dx_chains_pair(stat, par, ma[e], mb[e], qa[e], qb[e], C[e]);
    ChV<V>::st(a.out + i, r);
}

__global__ __launch_bounds__(BLOCK) void k_chains_pair(ChainsPairArgs a, DxChainsPar par, long long n, int stat) {
    const uintptr_t ao = addr(a.out);
    uintptr_t diff = ao & 7;
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        diff |= (ao ^ addr(a.ma[k])) | (ao ^ addr(a.mb[k])) | (ao ^ addr(a.qa[k])) | (ao ^ addr(a.qb[k])) | (ao ^ addr(a.C[k]));
    });
    // element by element where the two planes (or a chain's adopted buffers) are at different 16-byte phases
    dx_stream(n, (diff & 15) == 0, ao, [&](long long i) { chains_pair_item<1>(a, par, stat, i); },
              [&](long long i) { chains_pair_item<2>(a, par, stat, i); });
}

struct ChainsAngleArgs {
    const double* C[DX_CHAINS_MAX];
    const double* S[DX_CHAINS_MAX];
    double* out;
};

template <int V>
__device__ __forceinline__ void chains_angle_item(const ChainsAngleArgs& a, const DxAngPar& par, int stat, long long i) {
    double C[V][DX_CHAINS_MAX] = {}, S[V][DX_CHAINS_MAX] = {};
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        double vc[V], vs[V];
        ChV<V>::ld(a.C[k] + i, vc); ChV<V>::ld(a.S[k] + i, vs);
#pragma unroll
        for (int e = 0; e < V; ++e) { C[e][k] = vc[e]; S[e][k] = vs[e]; }
    });
    double r[V];
#pragma unroll
    for (int e = 0; e < V; ++e) r[e] = dx_angle_chains_stat(stat, par, C[e], S[e]);
    ChV<V>::st(a.out + i, r);
}

// the polarisation angle over several chains (dx_angle_host.h): the chains' Cbar, Sbar pooled by their sample counts and read as
// one chain's, or (stat 5) the circular std of the chains' mean directions
__global__ __launch_bounds__(BLOCK) void k_chains_angle(ChainsAngleArgs a, DxAngPar par, long long n, int stat) {
    const uintptr_t ao = addr(a.out);
    uintptr_t diff = ao & 7;
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        diff |= (ao ^ addr(a.C[k])) | (ao ^ addr(a.S[k]));
    });
    dx_stream(n, (diff & 15) == 0, ao, [&](long long i) { chains_angle_item<1>(a, par, stat, i); },
              [&](long long i) { chains_angle_item<2>(a, par, stat, i); });
}

struct ChainsHistArgs {
    const uint32_t* rec[DX_CHAINS_MAX];
    double q[DX_HIST_MAX_Q];
    double* out;          // [nq][n] (stat 0) or [n]
    double lo, hi;
    long long n;
    int K, nbins, bits, stat, nq;
};

// hist_walk over the SUM of the K records of pixel i: a 16-byte piece of every chain, its 4 or 8 counters summed in 64 bits,
// then f(count, bin) per bin in bin order until f says stop
// (A: ChainsHistArgs or ChainsRankArgs -- rec, K, bits)
template <class A, class F>
__device__ __forceinline__ void chains_hist_walk(const A& a, long long i, int pieces, F f) {
    int b = 0;
    for (int p = 0; p < pieces; ++p) {
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < DX_CHAINS_MAX; ++k)
            if (k < a.K) {
                const u32x4 v = ((const GU4*)a.rec[k])[i * pieces + p];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (a.bits == 16) { c[2 * j] += w[j] & 0xffffu; c[2 * j + 1] += w[j] >> 16; }
                    else c[j] += w[j];
                }
            }
        const int nb = a.bits == 16 ? 8 : 4;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nb && f(c[j], b + j)) return;
        b += nb;
    }
}

__global__ __launch_bounds__(BLOCK) void k_chains_hist(ChainsHistArgs a) {
    const int pieces = dx_hist_words(a.nbins, a.bits) / 4;
    dx_hist_readout<unsigned long long>(a, [&](long long i, auto f) { chains_hist_walk(a, i, pieces, f); });
}

struct ChainsHistPxArgs : ChainsHistArgs {
    const double* lo_map;   // [n]: the registration's range maps (chain 0's: the same in every chain) in place of lo, hi
    const double* hi_map;
};

// k_chains_hist of a registration with per-pixel ranges (quantiles and the mode; N needs no range and goes through k_chains_hist)
__global__ __launch_bounds__(BLOCK) void k_chains_hist_px(ChainsHistPxArgs a) {
    const int pieces = dx_hist_words(a.nbins, a.bits) / 4;
    dx_hist_readout_impl<true, unsigned long long>(a, [&](long long i, auto f) { chains_hist_walk(a, i, pieces, f); });
}

struct ChainsRankArgs {
    const uint32_t* rec[DX_CHAINS_MAX];
    double* out;          // [n]
    long long n;
    int K, nbins, bits, stat;
};

// the rank-normalised R-hat of pixel i (S > 0 pooled samples): chains_hist_walk with every chain's piece kept, so that a non-empty
// bin's score is formed once and goes into the triples of the chains that hold samples of it.  raw[k] and the triples are
// indexed by constants only (the k and j loops are unrolled): registers, no scratch
__device__ __forceinline__ double chains_rank_bulk(const ChainsRankArgs& a, long long i, int pieces, unsigned long long S) {
    DxRankState s;
    dx_rank_reset(s);
    unsigned long long cum = 0;
    const int nb = a.bits == 16 ? 8 : 4;
    for (int p = 0; p < pieces; ++p) {
        u32x4 raw[DX_CHAINS_MAX];
        unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < DX_CHAINS_MAX; ++k)
            if (k < a.K) {
                raw[k] = ((const GU4*)a.rec[k])[i * pieces + p];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (a.bits == 16) { c[2 * j] += raw[k][j] & 0xffffu; c[2 * j + 1] += raw[k][j] >> 16; }
                    else c[j] += raw[k][j];
                }
            }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nb)
                dx_rank_bin(a.K, c[j], cum, S, s, [&](auto kc) -> unsigned long long {
                    const u32x4 v = raw[decltype(kc)::value];
                    return a.bits == 16 ? (v[j >> 1] >> ((j & 1) * 16)) & 0xffffu : v[j & 3];
                });
    }
    return dx_rank_finish(a.K, s);
}

// A lane per pixel.  The walks after the first hit the cache lines the first brought in; the fold reads its counters by 32-bit
// word at m +- e (dx_hist_count), m being known only after the second walk.
__global__ __launch_bounds__(BLOCK) void k_chains_rank(ChainsRankArgs a) {
    const int words = dx_hist_words(a.nbins, a.bits), pieces = words / 4;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
        unsigned long long S = 0;
        int first = -1, last = -1;
        chains_hist_walk(a, i, pieces, [&](unsigned long long c, int b) { dx_rank_total_step(c, b, S, first, last); return false; });
        double r = (double)NAN;
        if (S > 0) {
            double bulk = 0.0, folded = 0.0;
            if (a.stat != DX_RK_FOLDED) bulk = chains_rank_bulk(a, i, pieces, S);
            if (a.stat != DX_RK_BULK) {
                unsigned long long cum = 0;
                int m = 0;
                const double half = 0.5 * (double)S;
                chains_hist_walk(a, i, pieces, [&](unsigned long long c, int b) { return dx_rank_median_step(c, b, half, cum, m); });
                folded = dx_rank_folded_of(a.K, a.nbins, m, first, last, S, [&](auto kc, int b) {   // 0 <= b < nbins: inside pixel i's record
                    return dx_hist_count(a.rec[decltype(kc)::value] + i * words, b, a.bits);
                });
            }
            r = a.stat == DX_RK_BULK ? bulk : a.stat == DX_RK_FOLDED ? folded : dx_rank_larger(bulk, folded);
        }
        a.out[i] = r;
    }
}

struct ChainsBatchArgs {   // one base pointer per chain (slot 0's mean plane of the registration) plus the stride of the regular layout
    const double* base[DX_CHAINS_MAX];
    double* out;
    long long pitch, n;
    DxBatchPar par;
};
static_assert(sizeof(ChainsBatchArgs) <= 2048, "the arguments must stay well inside the 4 KB kernel-argument segment");

// read where the kernel arguments lie (scalar loads at a computed offset: base[k], the ratio tables), never copied
typedef const ChainsBatchArgs __attribute__((address_space(4))) * batch_kptr;

template <int V>
__device__ __forceinline__ void chains_batch_item(batch_kptr a, long long i) {
    double r[V];
    const long long pitch = a->pitch;
    dx_chains_batches_stat<V>(a->par, [&](int k, int b, bool want_m2, double (&m)[V], double (&q)[V]) DX_LAMBDA_INLINE {
        const double* base = a->base[k];
        ChV<V>::ld(base + (2LL * b) * pitch + i, m);
        if (want_m2) ChV<V>::ld(base + (2LL * b + 1) * pitch + i, q);
        else {
#pragma unroll
            for (int e = 0; e < V; ++e) q[e] = 0.0;
        }
    }, r);
    ChV<V>::st(a->out + i, r);
}

// k_batches_stat over K chains: every chain's slots in one pass with running values, at most (2 K nbatch + 1) x 8 B per element;
// the 2K half-means of split R-hat stay in registers (constant subscripts through dx_chains_each)
// ChainsBatchArgs must stay the FIRST and ONLY explicit parameter: the kernel reads it at offset 0 of the kernel-argument segment,
// not through the (unnamed) parameter.  A parameter put in front of it would shift what `a` points at; one added behind it is
// harmless but must be read the same way or by name.
__global__ __launch_bounds__(BLOCK) void k_chains_batches(ChainsBatchArgs) {
    const batch_kptr a = (batch_kptr)__builtin_amdgcn_kernarg_segment_ptr();
    const uintptr_t ao = addr(a->out);
    uintptr_t diff = ao & 7;
    for (int k = 0; k < a->par.K; ++k) diff |= (ao ^ addr(a->base[k])) & 15;
    dx_stream(a->n, diff == 0, ao, [&](long long i) { chains_batch_item<1>(a, i); }, [&](long long i) { chains_batch_item<2>(a, i); });
}

// ---- host side

struct ChainSet {
    dangx_ctx* const* c;
    int K;
    long long cnt[DX_CHAINS_MAX];
};

int chains_fail(dangx_ctx* const* ctxs, const std::string& msg) { return fail(ctxs[0], "posterior chains: " + msg); }

// a holder (dangx_moments_begin_like) that was not given the section a read-out needs: refused before anything is launched
int chains_missing(dangx_ctx* const* ctxs, int k, const std::string& section) {
    return chains_fail(ctxs, "chain " + std::to_string(k) + ": section " + section + " was not put into this holder (dangx_moments_section_put)");
}

std::string planes_section(int comp, int what) { return "PLANES(" + std::to_string(comp) + ", " + std::to_string(what) + ")"; }

// the checks every read-out shares; on success cs describes the set
int chains_open(dangx_ctx* const* ctxs, int nchains, ChainSet& cs) {
    if (!ctxs || !ctxs[0]) return 1;
    if (nchains < 2 || nchains > DX_CHAINS_MAX)
        return chains_fail(ctxs, "nchains must be 2 .. DANGX_MAX_CHAINS (" + std::to_string(DX_CHAINS_MAX) + "), not " + std::to_string(nchains));
    for (int k = 1; k < nchains; ++k)
        if (!ctxs[k]) return chains_fail(ctxs, "chain " + std::to_string(k) + " is a null context");
    const dangx_ctx* c0 = ctxs[0];
    for (int k = 1; k < nchains; ++k) {
        const dangx_ctx* c = ctxs[k];
        const std::string at = "chain " + std::to_string(k);
        for (int o = 0; o < k; ++o)
            if (ctxs[o] == c) return chains_fail(ctxs, at + " is the same context as chain " + std::to_string(o) + " (a context listed twice)");
        if (c->device != c0->device)
            return chains_fail(ctxs, at + " lives on device " + std::to_string(c->device) + ", chain 0 on device " + std::to_string(c0->device) +
                                         ": chains on different devices are not supported");
        if (c->dims.npix != c0->dims.npix || c->dims.pix0 != c0->dims.pix0 || c->dims.nmaps != c0->dims.nmaps)
            return chains_fail(ctxs, at + " differs from chain 0 in npix / pix0 / nmaps");
    }
    for (int k = 0; k < nchains; ++k) {
        if (!ctxs[k]->mom) return chains_fail(ctxs, "chain " + std::to_string(k) + ": dangx_moments_begin was not called");
        if (ctxs[k]->mom->holder && !ctxs[k]->mom->head_put) return chains_missing(ctxs, k, "HEAD");
        if (ctxs[k]->mom->count == 0) return chains_fail(ctxs, "chain " + std::to_string(k) + ": no sample accumulated");
        cs.cnt[k] = ctxs[k]->mom->count;
    }
    cs.c = ctxs;
    cs.K = nchains;
    return 0;
}

int chains_counts(const ChainSet& cs, int stat, int ddof, bool is_pair) {
    const std::string why = dx_chains_count_check(cs.K, cs.cnt, stat, ddof, is_pair);
    return why.empty() ? 0 : chains_fail(cs.c, why);
}

int chains_need_lag(const ChainSet& cs) {
    for (int k = 0; k < cs.K; ++k)
        if (!cs.c[k]->mom->lag1)
            return chains_fail(cs.c, "chain " + std::to_string(k) + ": the lag-1 autocorrelation is not tracked (dangx_moments_pairs with lag1 != 0 was not called)");
    return 0;
}

// the selected planes of (comp, what): those of chain 0, which every other chain must have selected too
int chains_planes(const ChainSet& cs, int comp, int what, int stat, unsigned& planes) {
    if (what < 0 || what > DANGX_MAX_IND) return chains_fail(cs.c, "what must be 0 (amplitude) or 1 + index number");
    if (stat < DX_CH_MEAN || stat > DX_CH_ESS)
        return chains_fail(cs.c, "stat must be 0 (pooled mean), 1 (pooled std), 2 (R-hat), 3 (W), 4 (B/n) or 5 (pooled ESS)");
    for (int k = 0; k < cs.K; ++k) {
        const dangx_ctx* c = cs.c[k];
        if (comp < 0 || comp >= c->dims.ncomp) return chains_fail(cs.c, "chain " + std::to_string(k) + ": component index out of range");
        const unsigned pk = (unsigned)(c->mom->sel[comp] >> (what == 0 ? 0 : 3 + 3 * (what - 1))) & 7u;
        if (k == 0) planes = pk;
        if (!pk || (pk & planes) != planes)
            return chains_fail(cs.c, "chain " + std::to_string(k) + ": a plane of this component and what is not selected");
        if (is_global_type(c->desc[comp].type) != is_global_type(cs.c[0]->desc[comp].type))
            return chains_fail(cs.c, "chain " + std::to_string(k) + ": the component is of another kind than in chain 0");
    }
    if (stat == DX_CH_ESS && chains_need_lag(cs)) return 1;
    return 0;
}

// every other chain's stream before stream 0 ...
int chains_join(const ChainSet& cs) {
    dangx_ctx* c0 = cs.c[0];
    for (int k = 1; k < cs.K; ++k) {
        dangx_ctx* c = cs.c[k];
        if (c->stream == c0->stream) continue;
        DxMoments* m = c->mom;
        if (!m->chain_ev) HIPCHK(c0, hipEventCreateWithFlags(&m->chain_ev, hipEventDisableTiming));
        HIPCHK(c0, hipEventRecord(m->chain_ev, c->stream));
        HIPCHK(c0, hipStreamWaitEvent(c0->stream, m->chain_ev, 0));
    }
    return 0;
}

// ... and stream 0 before whatever the other streams do next: a following accumulation cannot overwrite what the kernel reads
int chains_release(const ChainSet& cs) {
    dangx_ctx* c0 = cs.c[0];
    DxMoments* m0 = c0->mom;
    bool any = false;
    for (int k = 1; k < cs.K; ++k) any = any || cs.c[k]->stream != c0->stream;
    if (!any) return 0;
    if (!m0->chain_ev) HIPCHK(c0, hipEventCreateWithFlags(&m0->chain_ev, hipEventDisableTiming));
    HIPCHK(c0, hipEventRecord(m0->chain_ev, c0->stream));
    for (int k = 1; k < cs.K; ++k)
        if (cs.c[k]->stream != c0->stream) HIPCHK(c0, hipStreamWaitEvent(cs.c[k]->stream, m0->chain_ev, 0));
    return 0;
}

// one launch on stream 0 between the two joins, timed as DANGX_K_CHAINS
template <class Launch>
int chains_run(const ChainSet& cs, Launch launch) {
    dangx_ctx* c0 = cs.c[0];
    if (chains_join(cs)) return 1;
    {
        Timed tm(c0, DANGX_K_CHAINS);
        launch();
        HIPCHK(c0, hipGetLastError());
    }
    return chains_release(cs);
}

// k_chains_stat on stream 0 between the two joins; a.mean .. a.out of np planes are filled in
int chains_launch(const ChainSet& cs, const ChainsArgs& a, int np, int stat, int ddof) {
    dangx_ctx* c0 = cs.c[0];
    const long long n = c0->dims.npix;
    const DxChainsPar par = dx_chains_par(cs.K, cs.cnt, ddof);
    return chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_stat, dim3(c0->mom->grid_for((n + 1) / 2, np), np), dim3(BLOCK), 0, c0->stream, a, par, n, stat); });
}

// Every read-out is one implementation; `out` is a device buffer, or with to_host a host array staged through chain 0 (ReadOut).
int chains_get_impl(dangx_ctx* const* ctxs, int nchains, int comp, int what, int stat, int ddof, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    unsigned planes = 0;
    if (chains_open(ctxs, nchains, cs) || chains_planes(cs, comp, what, stat, planes) || chains_counts(cs, stat, ddof, false)) return 1;
    dangx_ctx* c0 = ctxs[0];
    if (what == 0 && is_global_type(c0->desc[comp].type))
        return chains_fail(ctxs, "a template / monopole / hi_fit amplitude is read with dangx_chains_get_template");
    (void)hipSetDevice(c0->device);
    const long long np = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)np * c0->dims.nmaps)) return 1;
    ChainsArgs a{};
    int n = 0;
    for (int k = 0; k < c0->dims.nmaps; ++k) {
        if (!((planes >> k) & 1u)) continue;
        for (int j = 0; j < cs.K; ++j) {
            const DxMoments* m = ctxs[j]->mom;
            const int i = m->find_seg(comp, what, k);
            if (i < 0) return chains_fail(ctxs, "chain " + std::to_string(j) + ": a plane of this component and what is not selected");
            const auto& s = m->segs[i];
            a.mean[n][j] = m->mean(s);
            a.m2[n][j] = m->m2(s);
            if (stat == DX_CH_ESS) { a.prev[n][j] = m->prev(s); a.first[n][j] = m->first(s); a.P[n][j] = m->P(s); }
            if (!a.mean[n][j] || !a.m2[n][j]) return chains_missing(ctxs, j, planes_section(comp, what));
            if (stat == DX_CH_ESS && (!a.prev[n][j] || !a.first[n][j] || !a.P[n][j]))
                return chains_missing(ctxs, j, planes_section(comp, what) + " with its lag-1 parts");
        }
        a.out[n] = ro.dst + (long long)k * np;
        ++n;
    }
    if (chains_launch(cs, a, n, stat, ddof)) return 1;
    return ro.close(planes, c0->dims.nmaps, np, c0->host_stride > 0 ? c0->host_stride : np);
}

int chains_signal_impl(dangx_ctx* const* ctxs, int nchains, int sig, int stat, int ddof, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    if (stat < DX_CH_MEAN || stat > DX_CH_BN)
        return chains_fail(ctxs, "the stat of a signal must be 0 (pooled mean), 1 (pooled std), 2 (R-hat), 3 (W) or 4 (B/n)");
    const auto& s0 = ctxs[0]->mom->sigs;
    if (sig < 0 || sig >= (int)s0.size())
        return chains_fail(ctxs, "chain 0: signal index out of range (" + std::to_string(s0.size()) + " signals registered)");
    for (int k = 1; k < nchains; ++k) {
        const auto& sk = ctxs[k]->mom->sigs;
        if (sig >= (int)sk.size() || sk[sig].comp != s0[sig].comp || sk[sig].band != s0[sig].band || sk[sig].kind != s0[sig].kind)
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": signal " + std::to_string(sig) + " is not the registration of chain 0");
    }
    if (chains_counts(cs, stat, ddof, false)) return 1;
    dangx_ctx* c0 = ctxs[0];
    (void)hipSetDevice(c0->device);
    const long long n = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    ChainsArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        const DxMoments* m = ctxs[j]->mom;
        a.mean[0][j] = m->mean(m->sigs[sig]);
        a.m2[0][j] = m->m2(m->sigs[sig]);
        if (!a.mean[0][j]) return chains_missing(ctxs, j, "SIGNAL(" + std::to_string(sig) + ")");
    }
    a.out[0] = ro.dst;
    if (chains_launch(cs, a, 1, stat, ddof)) return 1;
    return ro.close(n);
}

// a fit item (dangx_moments_fit) over the chains: the signals' read-out on the item's (mean, m2)
int chains_fit_impl(dangx_ctx* const* ctxs, int nchains, int item, int stat, int ddof, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    if (stat < DX_CH_MEAN || stat > DX_CH_BN)
        return chains_fail(ctxs, "the stat of a fit item must be 0 (pooled mean), 1 (pooled std), 2 (R-hat), 3 (W) or 4 (B/n)");
    const auto& f0 = ctxs[0]->mom->fits;
    if (item < 0 || item >= (int)f0.size())
        return chains_fail(ctxs, "chain 0: fit item out of range (" + std::to_string(f0.size()) + " fit items registered)");
    for (int k = 1; k < nchains; ++k) {
        const auto& fk = ctxs[k]->mom->fits;
        if (item >= (int)fk.size() || fk[item].what != f0[item].what || fk[item].band != f0[item].band || fk[item].plane != f0[item].plane)
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": fit item " + std::to_string(item) + " is not the registration of chain 0");
    }
    if (chains_counts(cs, stat, ddof, false)) return 1;
    dangx_ctx* c0 = ctxs[0];
    (void)hipSetDevice(c0->device);
    const long long n = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    ChainsArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        const DxMoments* m = ctxs[j]->mom;
        a.mean[0][j] = m->mean(m->fits[item]);
        a.m2[0][j] = m->m2(m->fits[item]);
        if (!a.mean[0][j]) return chains_missing(ctxs, j, "FIT(" + std::to_string(item) + ")");
    }
    a.out[0] = ro.dst;
    if (chains_launch(cs, a, 1, stat, ddof)) return 1;
    return ro.close(n);
}

int chains_angle_impl(dangx_ctx* const* ctxs, int nchains, int ang, int stat, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    const std::string why = dx_angle_stat_check(stat, nchains);
    if (!why.empty()) return chains_fail(ctxs, why);
    const auto& a0 = ctxs[0]->mom->angs;
    if (ang < 0 || ang >= (int)a0.size())
        return chains_fail(ctxs, "chain 0: angle index out of range (" + std::to_string(a0.size()) + " angles registered)");
    for (int k = 1; k < nchains; ++k) {
        const auto& ak = ctxs[k]->mom->angs;
        if (ang >= (int)ak.size() || ak[ang].comp != a0[ang].comp || ak[ang].band != a0[ang].band)
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": angle " + std::to_string(ang) + " is not the registration of chain 0");
    }
    dangx_ctx* c0 = ctxs[0];
    (void)hipSetDevice(c0->device);
    const long long n = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    ChainsAngleArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        const DxMoments* m = ctxs[j]->mom;
        a.C[j] = m->angC(m->angs[ang]);
        a.S[j] = m->angS(m->angs[ang]);
        if (!a.C[j] || !a.S[j]) return chains_missing(ctxs, j, "ANGLE(" + std::to_string(ang) + ")");
    }
    a.out = ro.dst;
    const DxAngPar par = dx_angle_par(cs.K, cs.cnt);
    if (chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_angle, dim3(c0->mom->grid_for((n + 1) / 2, 1)), dim3(BLOCK), 0, c0->stream, a, par, n, stat); })) return 1;
    return ro.close(n);
}

int chains_pair_impl(dangx_ctx* const* ctxs, int nchains, int pair, int stat, int ddof, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    if (stat != 0 && stat != 1) return chains_fail(ctxs, "the stat of a pair must be 0 (covariance) or 1 (correlation)");
    const DxMoments* m0 = ctxs[0]->mom;
    if (pair < 0 || pair >= (int)m0->pairs.size())
        return chains_fail(ctxs, "chain 0: pair index out of range (" + std::to_string(m0->pairs.size()) + " pairs registered)");
    for (int k = 1; k < nchains; ++k) {
        const DxMoments* m = ctxs[k]->mom;
        if (pair >= (int)m->pairs.size() || !same_plane(m->segs[m->pairs[pair].a], m0->segs[m0->pairs[pair].a]) ||
            !same_plane(m->segs[m->pairs[pair].b], m0->segs[m0->pairs[pair].b]))
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": pair " + std::to_string(pair) + " is not the registration of chain 0");
    }
    if (chains_counts(cs, stat, ddof, true)) return 1;
    dangx_ctx* c0 = ctxs[0];
    (void)hipSetDevice(c0->device);
    const long long n = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    ChainsPairArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        const DxMoments* m = ctxs[j]->mom;
        const auto& p = m->pairs[pair];
        const auto &sa = m->segs[p.a], &sb = m->segs[p.b];
        a.ma[j] = m->mean(sa); a.mb[j] = m->mean(sb);
        a.qa[j] = m->m2(sa); a.qb[j] = m->m2(sb);
        a.C[j] = m->C(p);
        if (!a.C[j]) return chains_missing(ctxs, j, "PAIR(" + std::to_string(pair) + ")");
        if (!a.ma[j] || !a.qa[j]) return chains_missing(ctxs, j, planes_section(sa.comp, sa.what));
        if (!a.mb[j] || !a.qb[j]) return chains_missing(ctxs, j, planes_section(sb.comp, sb.what));
    }
    a.out = ro.dst;
    const DxChainsPar par = dx_chains_par(cs.K, cs.cnt, ddof);
    if (chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_pair, dim3(c0->mom->grid_for((n + 1) / 2, 1)), dim3(BLOCK), 0, c0->stream, a, par, n, stat); })) return 1;
    return ro.close(n);
}

// histogram registration reg is the same in every chain (after chains_open)
int chains_hist_same(dangx_ctx* const* ctxs, int nchains, int reg) {
    const DxMoments* m0 = ctxs[0]->mom;
    if (reg < 0 || reg >= (int)m0->hists.size())
        return chains_fail(ctxs, "chain 0: histogram registration out of range (" + std::to_string(m0->hists.size()) + " registered)");
    for (int k = 1; k < nchains; ++k) {
        const DxMoments* m = ctxs[k]->mom;
        bool same = reg < (int)m->hists.size() && m->hbins == m0->hbins && m->hbits == m0->hbits;
        if (same) {
            const auto &h = m->hists[reg], &h0 = m0->hists[reg];
            same = h.sig == h0.sig && (h.sig >= 0 || same_plane(m->segs[h.seg], m0->segs[h0.seg])) && h.lo == h0.lo && h.hi == h0.hi && h.kind == h0.kind && h.sum == h0.sum;
        }
        if (!same)
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": histogram registration " + std::to_string(reg) +
                                         " is not the registration of chain 0 (plane, lo, hi, nbins and bits must agree, and with per-pixel "
                                         "ranges the checksum of the range maps)");
    }
    return 0;
}

int chains_hist_impl(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int nq, const double* q, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs) || chains_hist_same(ctxs, nchains, reg)) return 1;
    const DxMoments* m0 = ctxs[0]->mom;
    dangx_ctx* c0 = ctxs[0];
    if (dx_hist_stat_check(c0, reg, stat, nq, q)) return 1;
    (void)hipSetDevice(c0->device);
    const long long total = (long long)c0->dims.npix * (stat == 0 ? nq : 1);
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)total)) return 1;
    ChainsHistArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        a.rec[j] = ctxs[j]->mom->records(ctxs[j]->mom->hists[reg]);
        if (!a.rec[j]) return chains_missing(ctxs, j, "HIST(" + std::to_string(reg) + ")");
    }
    a.out = ro.dst; a.lo = m0->hists[reg].lo; a.hi = m0->hists[reg].hi; a.n = c0->dims.npix;
    a.K = cs.K; a.nbins = m0->hbins; a.bits = m0->hbits; a.stat = stat; a.nq = stat == 0 ? nq : 0;
    for (int j = 0; j < a.nq; ++j) a.q[j] = q[j];
    const auto& h0 = m0->hists[reg];
    if (h0.kind == DX_HIST_RANGE_PIXEL && stat != 2) {   // quantiles and the mode need the pixels' bounds (chain 0's maps); N does not
        ChainsHistPxArgs ap{};
        static_cast<ChainsHistArgs&>(ap) = a;
        ap.lo_map = m0->range_lo(h0); ap.hi_map = m0->range_hi(h0);
        if (!ap.lo_map) return chains_missing(ctxs, 0, "HIST_RANGE(" + std::to_string(reg) + ")");
        if (chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_hist_px, dim3(c0->mom->grid_for(a.n, 1)), dim3(BLOCK), 0, c0->stream, ap); })) return 1;
        return ro.close(total);
    }
    if (chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_hist, dim3(c0->mom->grid_for(a.n, 1)), dim3(BLOCK), 0, c0->stream, a); })) return 1;
    return ro.close(total);
}

int chains_rank_impl(dangx_ctx* const* ctxs, int nchains, int reg, int stat, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs) || chains_hist_same(ctxs, nchains, reg)) return 1;
    const DxMoments* m0 = ctxs[0]->mom;
    dangx_ctx* c0 = ctxs[0];
    if (dx_hist_stat_check(c0, reg, 2, 0, nullptr)) return 1;   // the registration and the sample count, as for a pooled count
    const std::string why = dx_rank_check(cs.K, m0->hbins, m0->hbits, stat);
    if (!why.empty()) return chains_fail(ctxs, "dangx_chains_hist_rank: " + why);
    (void)hipSetDevice(c0->device);
    const long long n = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    ChainsRankArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        a.rec[j] = ctxs[j]->mom->records(ctxs[j]->mom->hists[reg]);
        if (!a.rec[j]) return chains_missing(ctxs, j, "HIST(" + std::to_string(reg) + ")");
    }
    a.out = ro.dst; a.n = n; a.K = cs.K; a.nbins = m0->hbins; a.bits = m0->hbits; a.stat = stat;
    if (chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_rank, dim3(c0->mom->grid_for(n, 1)), dim3(BLOCK), 0, c0->stream, a); })) return 1;
    return ro.close(n);
}

int chains_batches_impl(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int first, int ddof, double* out, bool to_host) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    const DxMoments* m0 = ctxs[0]->mom;
    if (m0->batches.empty()) return chains_fail(ctxs, "chain 0: no batches are registered (dangx_moments_batches was not called)");
    if (reg < 0 || reg >= (int)m0->batches.size())
        return chains_fail(ctxs, "chain 0: batch registration out of range (" + std::to_string(m0->batches.size()) + " registered)");
    for (int k = 1; k < nchains; ++k) {
        const DxMoments* m = ctxs[k]->mom;
        const std::string at = "chain " + std::to_string(k) + ": ";
        if (reg >= (int)m->batches.size() || !same_plane(m->segs[m->batches[reg].seg], m0->segs[m0->batches[reg].seg]))
            return chains_fail(ctxs, at + "batch registration " + std::to_string(reg) + " is not the registration of chain 0");
        if (m->nbatch != m0->nbatch)
            return chains_fail(ctxs, at + "nbatch is " + std::to_string(m->nbatch) + ", chain 0 has " + std::to_string(m0->nbatch));
        if (m->count != m0->count)
            return chains_fail(ctxs, at + "batch read-outs need equal sample counts: it holds " + std::to_string(m->count) + ", chain 0 holds " +
                                         std::to_string(m0->count));
        if (m->batch_len != m0->batch_len)
            return chains_fail(ctxs, at + "the batch length is " + std::to_string(m->batch_len) + ", chain 0 has " + std::to_string(m0->batch_len));
    }
    const DxBatchPos p = dx_batches_pos(m0->count, m0->batch_len);
    std::string why = dx_batches_stat_check(stat, first, 0, p.L, p.nfull, p.partial);
    if (why.empty() && stat == DX_BT_STD) {
        const long long N = (long long)nchains * ((p.nfull - first) * p.L + p.partial);
        if (ddof < 0 || N - ddof <= 0) why = "standard deviation needs 0 <= ddof < N (N = " + std::to_string(N) + ")";
    }
    if (!why.empty()) return chains_fail(ctxs, "dangx_chains_batches_get: " + why);
    dangx_ctx* c0 = ctxs[0];
    (void)hipSetDevice(c0->device);
    const long long n = c0->dims.npix;
    ReadOut ro{c0, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    ChainsBatchArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        a.base[j] = ctxs[j]->mom->bmean(ctxs[j]->mom->batches[reg], 0);
        if (!a.base[j]) return chains_missing(ctxs, j, "BATCHES(" + std::to_string(reg) + ")");
    }
    a.out = ro.dst; a.pitch = m0->bpitch; a.n = n;
    a.par = dx_batches_par(stat, first, ddof, p.L, p.nfull, p.partial, cs.K);
    if (chains_run(cs, [&] { hipLaunchKernelGGL(k_chains_batches, dim3(c0->mom->grid_for((n + 1) / 2, 1)), dim3(BLOCK), 0, c0->stream, a); })) return 1;
    return ro.close(n);
}

}  // namespace

extern "C" {

int dangx_chains_batches_get_dev(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int first, int ddof, double* out_dev) {
    return chains_batches_impl(ctxs, nchains, reg, stat, first, ddof, out_dev, false);
}

int dangx_chains_batches_get(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int first, int ddof, double* out) {
    return chains_batches_impl(ctxs, nchains, reg, stat, first, ddof, out, true);
}

int dangx_chains_get_dev(dangx_ctx* const* ctxs, int nchains, int comp, int what, int stat, int ddof, double* out_dev) {
    return chains_get_impl(ctxs, nchains, comp, what, stat, ddof, out_dev, false);
}

int dangx_chains_get(dangx_ctx* const* ctxs, int nchains, int comp, int what, int stat, int ddof, double* out) {
    return chains_get_impl(ctxs, nchains, comp, what, stat, ddof, out, true);
}

int dangx_chains_get_template(dangx_ctx* const* ctxs, int nchains, int comp, int stat, int ddof, double* ta) {
    if (!ctxs || !ctxs[0] || !ta) return 1;
    ChainSet cs{};
    unsigned planes = 0;
    if (chains_open(ctxs, nchains, cs) || chains_planes(cs, comp, 0, stat, planes) || chains_counts(cs, stat, ddof, false)) return 1;
    const dangx_ctx* c0 = ctxs[0];
    if (!is_global_type(c0->desc[comp].type)) return chains_fail(ctxs, "not a template / monopole / hi_fit component");
    for (int k = 1; k < nchains; ++k)
        if (ctxs[k]->dims.nbands != c0->dims.nbands) return chains_fail(ctxs, "chain " + std::to_string(k) + " differs from chain 0 in nbands");
    for (int k = 0; k < nchains; ++k)
        if (ctxs[k]->mom->holder && !ctxs[k]->mom->h_rows[comp]) return chains_missing(ctxs, k, planes_section(comp, 0));
    const DxChainsPar par = dx_chains_par(cs.K, cs.cnt, ddof);
    for (int k = 0; k < c0->dims.nmaps; ++k) {
        if (!((planes >> k) & 1u)) continue;
        for (int j = 0; j < c0->dims.nbands; ++j) {
            double v = 0.0;
            if (stat == DX_CH_ESS) {
                for (int i = 0; i < cs.K; ++i) {
                    const DxMoments* m = ctxs[i]->mom;
                    v = dx_chains_ess_add(v, m->tm_mean[comp][k][j], m->tm_m2[comp][k][j], m->tm_prev[comp][k][j], m->tm_first[comp][k][j],
                                          m->tm_P[comp][k][j], par.cnt[i]);
                }
            } else {
                double mean[DX_CHAINS_MAX] = {}, m2[DX_CHAINS_MAX] = {};
                for (int i = 0; i < cs.K; ++i) {
                    mean[i] = ctxs[i]->mom->tm_mean[comp][k][j];
                    m2[i] = ctxs[i]->mom->tm_m2[comp][k][j];
                }
                v = dx_chains_stat(stat, par, mean, m2);
            }
            ta[k * c0->dims.nbands + j] = v;
        }
    }
    return 0;
}

int dangx_chains_get_signal_dev(dangx_ctx* const* ctxs, int nchains, int sig, int stat, int ddof, double* out_dev) {
    return chains_signal_impl(ctxs, nchains, sig, stat, ddof, out_dev, false);
}

int dangx_chains_get_signal(dangx_ctx* const* ctxs, int nchains, int sig, int stat, int ddof, double* out) {
    return chains_signal_impl(ctxs, nchains, sig, stat, ddof, out, true);
}

int dangx_chains_get_fit_dev(dangx_ctx* const* ctxs, int nchains, int item, int stat, int ddof, double* out_dev) {
    return chains_fit_impl(ctxs, nchains, item, stat, ddof, out_dev, false);
}

int dangx_chains_get_fit(dangx_ctx* const* ctxs, int nchains, int item, int stat, int ddof, double* out) {
    return chains_fit_impl(ctxs, nchains, item, stat, ddof, out, true);
}

int dangx_chains_get_angle_dev(dangx_ctx* const* ctxs, int nchains, int ang, int stat, double* out_dev) {
    return chains_angle_impl(ctxs, nchains, ang, stat, out_dev, false);
}

int dangx_chains_get_angle(dangx_ctx* const* ctxs, int nchains, int ang, int stat, double* out) {
    return chains_angle_impl(ctxs, nchains, ang, stat, out, true);
}

int dangx_chains_get_pair_dev(dangx_ctx* const* ctxs, int nchains, int pair, int stat, int ddof, double* out_dev) {
    return chains_pair_impl(ctxs, nchains, pair, stat, ddof, out_dev, false);
}

int dangx_chains_get_pair(dangx_ctx* const* ctxs, int nchains, int pair, int stat, int ddof, double* out) {
    return chains_pair_impl(ctxs, nchains, pair, stat, ddof, out, true);
}

int dangx_chains_hist_stat_dev(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int nq, const double* q, double* out_dev) {
    return chains_hist_impl(ctxs, nchains, reg, stat, nq, q, out_dev, false);
}

int dangx_chains_hist_stat(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int nq, const double* q, double* out) {
    return chains_hist_impl(ctxs, nchains, reg, stat, nq, q, out, true);
}

int dangx_chains_hist_rank_dev(dangx_ctx* const* ctxs, int nchains, int reg, int stat, double* out_dev) {
    return chains_rank_impl(ctxs, nchains, reg, stat, out_dev, false);
}

int dangx_chains_hist_rank(dangx_ctx* const* ctxs, int nchains, int reg, int stat, double* out) {
    return chains_rank_impl(ctxs, nchains, reg, stat, out, true);
}

}  // extern "C"
