// dangx_moments.hip -- posterior moments of the chain state, accumulated in HBM (dangx_moments_*): the mean and standard deviation
// of every selected amplitude / index plane over the samples the driver hands in, without a map leaving the device until the end.
// The reference writes every sample with write_maps (src/dang.f90:119-121) and averages the FITS files afterwards
// (scripts/make_mean_maps.py: return_mean_map, return_std_map = np.std, ddof 0).
//
// k_moments_accum is one pass over every selected plane: Welford's update with the new sample count n (inv_n = 1/n from the host),
//     d = x - mean;  mean += d * inv_n;  m2 += d * (x - mean)
// in f64 accumulators [plane][npix] that dangx_moments_begin allocates.  It is a pure stream of 5 x 8 B per element (read x, mean,
// m2; write mean, m2) with 16-byte accesses; a plane whose x, mean and m2 do not share their 16-byte phase (an adopted buffer
// adopted again at another alignment) takes the scalar path, and so do the odd first / last element of every plane.  Both paths
// evaluate the same expression with explicit fma: results do not depend on which path an element takes, i.e. on the shard
// boundaries or the alignment of the caller's buffers.
//
// Template amplitudes of global-amplitude members (<= 3 x nbands values) live on the host (ctx->tamp, current after every call
// that samples them) and get the same update there: accumulation adds no device-to-host synchronisation.
//
// dangx_moments_pairs adds two second-order statistics, streams of the same shape (expressions in dx_moments_host.h):
//   lag-1 autocorrelation of every selected plane: k_moments_accum_lag replaces k_moments_accum and keeps, beside mean and m2, the
//     first sample r, the previous sample and P = sum (x_t - r)(x_{t-1} - r) -- one read of x, at most 10 x 8 B per element (read
//     x, mean, m2, prev, r, P; write mean, m2, prev, P).  The previous sample is written by the thread that read it.
//   cross terms of pairs of planes: k_moments_pairs, C += (a - mean_a_old)(b - mean_b_new) with mean_b_new formed in registers,
//     6 x 8 B per element (read a, b, both old means, C; write C).  It is a launch of its own BEFORE the launch that updates the
//     means (stream order), so no block reads a mean another block is writing.
// Without dangx_moments_pairs an accumulation is the one k_moments_accum launch, as before.
//
// dangx_moments_hist adds fixed-range per-pixel histograms of registered pixel planes (definitions in dx_hist_host.h): a record of
// nbins counters (<= 128 bytes, a power of two: never across a 128-byte request) per pixel and registration, in an allocation of
// the library's own.  k_moments_hist takes one sample of every registered plane in ONE launch of its own (blockIdx.y =
// registration) behind the moments': the thread that read a pixel's x loads, increments and stores the ONE 32-bit word holding the
// bin -- no atomics, a pixel's record belongs to one thread -- and a sample outside the range touches no record.  k_hist_stat
// reads a record as 16-byte pieces and leaves quantiles, the mode or the count of counted samples.  Nothing registered: no launch.
//
// dangx_moments_signals adds the moments of component signals at a band (definitions in dx_signal_host.h): the sample
// comp_signal(band, pix, plane) = amplitude * sed(indices) of a diffuse component -- what write_maps' output_fg maps hold
// (src/dang_data_mod.f90:596-617) -- and its polarised intensity P = sqrt(Q^2 + U^2), nonlinear in the sampled parameters and so not
// derivable from their moments.  k_moments_signal is a launch of its own behind the others (blockIdx.y = segment: a component
// and plane class with up to 8 bands): a thread reads a pixel's amplitude and index values once, prepares the SED once per plane
// and updates the f64 mean / m2 planes of every registered output of every band of the segment.  Segments with an integrated
// band go to a second launch of the kernel's BP form (the streaming form carries no bandpass code).  Nothing registered: no launch.
#include "dx_host.h"
#include "dx_moments_host.h"
#include "dx_hist_host.h"
#include "dx_signal_host.h"
#include "dx_chains_host.h"

#include <cstdint>

static_assert(DX_MOM_MAX_PAIRS == DANGX_MAX_PAIRS, "dx_moments_host.h and include/dangx.h disagree");
static_assert(DX_HIST_MAX == DANGX_MAX_HIST, "dx_hist_host.h and include/dangx.h disagree");
static_assert(DX_SIG_MAX == DANGX_MAX_SIGNALS, "dx_signal_host.h and include/dangx.h disagree");
static_assert(DX_CHAINS_MAX == DANGX_MAX_CHAINS, "dx_chains_host.h and include/dangx.h disagree");

struct MomSeg {           // one selected plane: the chain's plane (resolved at accumulate time) and its two accumulators
    const double* x;
    double* mean;
    double* m2;
    long long n;
};

struct LagSeg {           // a selected plane with lag-1 tracking: MomSeg + previous sample, first sample, P
    const double* x;
    double* mean;
    double* m2;
    double* prev;
    double* first;
    double* P;
    long long n;
};

struct PairSeg {          // a pair of selected planes and its cross-term accumulator
    const double* xa;
    const double* xb;
    const double* ma;
    const double* mb;
    double* C;
    long long n;
};

struct HistSeg {          // one registered histogram: the chain's plane (resolved at accumulate time) and its records
    const double* x;
    uint32_t* rec;        // [n][words] 32-bit words, 256-byte aligned
    double lo, hi, scale;
    long long n;
    int nbins, bits;
};

struct SigBand {          // one band of a signal segment: the accumulators of its outputs (slot 0..2: T, or Q, U, P), null = not wanted
    double* mean[3];
    double* m2[3];
    int band;
    unsigned want;        // bit o: output slot o is registered
};

struct SigSeg {           // a (component, plane class) with up to DX_SIG_SEG_BANDS bands; the chain's planes resolved at accumulate time
    const double* amp;    // the component's [nmaps][npix]: what the table is compared by
    const double* idx;    // the component's [nind][nmaps][npix]
    // src[k][0..2]: the amplitude and the two index planes of plane k of the class.  A plane the component does not have (an index
    // beyond nindices) or no output needs points at a plane that IS read: the load hits the cache and its value is never used
    const double* src[2][3];
    long long n;
    int comp, k0, np, nb; // k0: first plane (1-based) of the class, np: planes of the class (1: T, 2: Q+U)
    int vec, nind;        // nind: indices of the component (load_theta: an index beyond it is 0.0).  vec 0: element by element; 1 / 2: pairs of pixels, every plane read and every accumulator at 16-byte phase 0 / 8
    SigBand b[DX_SIG_SEG_BANDS];
};

struct DxMoments {
    int32_t sel[MAXC] = {};          // effective selection (bits as in include/dangx.h)
    int type[MAXC] = {}, nind[MAXC] = {};  // shape key recorded at begin
    struct Seg { int comp, what, plane; long long off; };
    std::vector<Seg> segs;
    std::vector<MomSeg> table;       // the table as last uploaded
    MomSeg* d_table = nullptr;
    double* acc = nullptr;           // [mean: acc_half doubles | m2: acc_half doubles]
    long long acc_half = 0;
    long long count = 0;
    double tm_mean[MAXC][3][MAXB] = {}, tm_m2[MAXC][3][MAXB] = {};
    double* scratch = nullptr;       // [nmaps][npix]: what the host getter copies from
    unsigned grid_target = 0;        // blocks of a full-machine launch
    // dangx_moments_pairs
    bool lag1 = false;
    double* lag = nullptr;           // [prev | first | P], acc_half doubles each, planes at the offsets of acc
    LagSeg* d_lag = nullptr;
    struct Pair { int a, b; long long off; };   // indices into segs; off: the pair's plane in pc (at the phase of a's mean)
    std::vector<Pair> pairs;
    double* pc = nullptr;
    PairSeg* d_pairs = nullptr;
    double tm_prev[MAXC][3][MAXB] = {}, tm_first[MAXC][3][MAXB] = {}, tm_P[MAXC][3][MAXB] = {};
    // dangx_moments_hist
    struct Hist { int seg; double lo, hi; long long off; };   // seg: index into segs; off: the records' first word in hrec
    std::vector<Hist> hists;
    int hbins = 0, hbits = 0;
    uint32_t* hrec = nullptr;        // every registration's records, each block at a multiple of 256 bytes
    HistSeg* d_hist = nullptr;
    double* hscratch = nullptr;      // what the host form of the read-out copies from
    size_t hscratch_bytes = 0;
    // dangx_moments_signals
    struct Sig { int comp, band, kind; long long off; };   // off: the signal's mean plane in sacc (its m2 plane: + sacc_half)
    std::vector<Sig> sigs;
    std::vector<DxSigSeg> sig_plan;
    int sig_type[MAXC] = {}, sig_nind[MAXC] = {};   // shape key of the registered components at registration
    bool sig_used[MAXC] = {};
    std::vector<SigSeg> sig_table;   // the table as last uploaded
    SigSeg* d_sig = nullptr;
    double* sacc = nullptr;          // [mean: sacc_half doubles | m2: sacc_half doubles]
    long long sacc_half = 0;
    // dangx_chains_*: orders this chain's stream against the stream of the chain set's first context (created on first use)
    hipEvent_t chain_ev = nullptr;
};

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) dbl2 GD2;   // two doubles in global memory

__device__ __forceinline__ void welford(double x, double& mean, double& m2, double inv_n) {
    const double d = x - mean;
    mean = fma(d, inv_n, mean);
    m2 = fma(d, x - mean, m2);
}

// blockIdx.y = segment; the blocks of a segment stride over its pairs of doubles
__global__ __launch_bounds__(BLOCK) void k_moments_accum(const MomSeg* __restrict__ segs, double inv_n) {
    const MomSeg s = segs[blockIdx.y];
    const long long n = s.n;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const uintptr_t ax = reinterpret_cast<uintptr_t>(s.x), am = reinterpret_cast<uintptr_t>(s.mean), a2 = reinterpret_cast<uintptr_t>(s.m2);
    if (((ax ^ am) & 15) != 0 || ((am ^ a2) & 15) != 0) {   // no common 16-byte phase: element by element
        for (long long i = gid; i < n; i += stride) {
            double m = s.mean[i], q = s.m2[i];
            welford(s.x[i], m, q, inv_n);
            s.mean[i] = m; s.m2[i] = q;
        }
        return;
    }
    const long long head = ((ax & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;   // tail < n: one element after the last pair
    if (gid == 0 && head) {
        double m = s.mean[0], q = s.m2[0];
        welford(s.x[0], m, q, inv_n);
        s.mean[0] = m; s.m2[0] = q;
    }
    if (gid == 1 && tail < n) {
        double m = s.mean[tail], q = s.m2[tail];
        welford(s.x[tail], m, q, inv_n);
        s.mean[tail] = m; s.m2[tail] = q;
    }
    // the table's pointers are generic: named global, the pairs load and store as global_load / global_store_dwordx4
    const GD2* __restrict__ x2 = (const GD2*)(s.x + head);
    GD2* __restrict__ m2v = (GD2*)(s.mean + head);
    GD2* __restrict__ q2v = (GD2*)(s.m2 + head);
    for (long long p = gid; p < npair; p += stride) {
        const dbl2 x = x2[p], m = m2v[p], q = q2v[p];
        double m0 = m.x, m1 = m.y, q0 = q.x, q1 = q.y;
        welford(x.x, m0, q0, inv_n);
        welford(x.y, m1, q1, inv_n);
        m2v[p] = dbl2{m0, m1}; q2v[p] = dbl2{q0, q1};
    }
}

// Welford's update and the lag-1 state from one read of x.  FIRST (sample 1): r = prev = x, P stays the 0 it was allocated with.
template <bool FIRST>
__device__ __forceinline__ void lag_step(double x, double& mean, double& m2, double& prev, double r, double& P, double inv_n) {
    if (FIRST) prev = x;
    else dx_lag_update(x, prev, r, P);
    welford(x, mean, m2, inv_n);
}

template <bool FIRST>
__device__ __forceinline__ void lag_one(const LagSeg& s, long long i, double inv_n) {
    const double x = s.x[i];
    double m = s.mean[i], q = s.m2[i], pv = 0.0, P = 0.0;
    if (!FIRST) { pv = s.prev[i]; P = s.P[i]; }
    lag_step<FIRST>(x, m, q, pv, FIRST ? x : s.first[i], P, inv_n);
    s.mean[i] = m; s.m2[i] = q; s.prev[i] = pv;
    if (FIRST) s.first[i] = x;
    else s.P[i] = P;
}

// k_moments_accum with the lag-1 state; the accumulators of a plane share their 16-byte phase by construction (dangx_moments_begin
// / _pairs), so as there only the chain's plane can be off phase
template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_moments_accum_lag(const LagSeg* __restrict__ segs, double inv_n) {
    const LagSeg s = segs[blockIdx.y];
    const long long n = s.n;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const uintptr_t ax = reinterpret_cast<uintptr_t>(s.x), am = reinterpret_cast<uintptr_t>(s.mean);
    const uintptr_t others = (am ^ reinterpret_cast<uintptr_t>(s.m2)) | (am ^ reinterpret_cast<uintptr_t>(s.prev)) |
                             (am ^ reinterpret_cast<uintptr_t>(s.first)) | (am ^ reinterpret_cast<uintptr_t>(s.P));
    if ((((ax ^ am) | others) & 15) != 0) {   // no common 16-byte phase: element by element
        for (long long i = gid; i < n; i += stride) lag_one<FIRST>(s, i, inv_n);
        return;
    }
    const long long head = ((ax & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;
    if (gid == 0 && head) lag_one<FIRST>(s, 0, inv_n);
    if (gid == 1 && tail < n) lag_one<FIRST>(s, tail, inv_n);
    const GD2* __restrict__ x2 = (const GD2*)(s.x + head);
    GD2* __restrict__ m2v = (GD2*)(s.mean + head);
    GD2* __restrict__ q2v = (GD2*)(s.m2 + head);
    GD2* __restrict__ pv2 = (GD2*)(s.prev + head);
    GD2* __restrict__ r2 = (GD2*)(s.first + head);
    GD2* __restrict__ P2 = (GD2*)(s.P + head);
    for (long long p = gid; p < npair; p += stride) {
        const dbl2 x = x2[p], m = m2v[p], q = q2v[p];
        double m0 = m.x, m1 = m.y, q0 = q.x, q1 = q.y;
        if (FIRST) {
            welford(x.x, m0, q0, inv_n);
            welford(x.y, m1, q1, inv_n);
            pv2[p] = x; r2[p] = x;
        } else {
            const dbl2 pv = pv2[p], r = r2[p], P = P2[p];
            double pv0 = pv.x, pv1 = pv.y, P0 = P.x, P1 = P.y;
            lag_step<false>(x.x, m0, q0, pv0, r.x, P0, inv_n);
            lag_step<false>(x.y, m1, q1, pv1, r.y, P1, inv_n);
            pv2[p] = dbl2{pv0, pv1}; P2[p] = dbl2{P0, P1};
        }
        m2v[p] = dbl2{m0, m1}; q2v[p] = dbl2{q0, q1};
    }
}

// blockIdx.y = pair.  Reads the means as the PREVIOUS accumulation left them: launched before the kernel that updates them.
__global__ __launch_bounds__(BLOCK) void k_moments_pairs(const PairSeg* __restrict__ segs, double inv_n) {
    const PairSeg s = segs[blockIdx.y];
    const long long n = s.n;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const uintptr_t ac = reinterpret_cast<uintptr_t>(s.C);
    const uintptr_t diff = (ac ^ reinterpret_cast<uintptr_t>(s.xa)) | (ac ^ reinterpret_cast<uintptr_t>(s.xb)) |
                           (ac ^ reinterpret_cast<uintptr_t>(s.ma)) | (ac ^ reinterpret_cast<uintptr_t>(s.mb));
    if ((diff & 15) != 0) {   // the two planes (or an adopted buffer) are at different 16-byte phases: element by element
        for (long long i = gid; i < n; i += stride) s.C[i] = dx_pair_update(s.xa[i], s.xb[i], s.ma[i], s.mb[i], s.C[i], inv_n);
        return;
    }
    const long long head = ((ac & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;
    if (gid == 0 && head) s.C[0] = dx_pair_update(s.xa[0], s.xb[0], s.ma[0], s.mb[0], s.C[0], inv_n);
    if (gid == 1 && tail < n) s.C[tail] = dx_pair_update(s.xa[tail], s.xb[tail], s.ma[tail], s.mb[tail], s.C[tail], inv_n);
    const GD2* __restrict__ a2 = (const GD2*)(s.xa + head);
    const GD2* __restrict__ b2 = (const GD2*)(s.xb + head);
    const GD2* __restrict__ ma2 = (const GD2*)(s.ma + head);
    const GD2* __restrict__ mb2 = (const GD2*)(s.mb + head);
    GD2* __restrict__ C2 = (GD2*)(s.C + head);
    for (long long p = gid; p < npair; p += stride) {
        const dbl2 a = a2[p], b = b2[p], ma = ma2[p], mb = mb2[p], c = C2[p];
        C2[p] = dbl2{dx_pair_update(a.x, b.x, ma.x, mb.x, c.x, inv_n), dx_pair_update(a.y, b.y, ma.y, mb.y, c.y, inv_n)};
    }
}

typedef __attribute__((address_space(1))) uint32_t GU32;   // a 32-bit word in global memory
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 GU4;      // a 16-byte piece of a record in global memory

// one sample into pixel i's record: the one word holding the bin is loaded, incremented and stored; outside the range, nothing.
// The 16-bit halves of a word belong to the same pixel and the host bounds the count by 2^bits - 1: no carry into the other half.
__device__ __forceinline__ void hist_one(const HistSeg& s, int words, long long i, double x) {
    if (!dx_hist_counted(x, s.lo, s.hi)) return;
    const int b = dx_hist_bin(x, s.lo, s.scale, s.nbins);
    GU32* w = (GU32*)s.rec + i * words + dx_hist_word_of(b, s.bits);
    *w = *w + dx_hist_one(b, s.bits);
}

// blockIdx.y = registration; x is read as the moments read it (pairs of doubles, the odd first / last element alone; a plane off
// the 16-byte grid shifts by its head element), the records are the library's own
__global__ __launch_bounds__(BLOCK) void k_moments_hist(const HistSeg* __restrict__ segs) {
    const HistSeg s = segs[blockIdx.y];
    const long long n = s.n;
    const int words = dx_hist_words(s.nbins, s.bits);
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const uintptr_t ax = reinterpret_cast<uintptr_t>(s.x);
    if ((ax & 7) != 0) {   // not even a double's alignment: element by element
        for (long long i = gid; i < n; i += stride) hist_one(s, words, i, s.x[i]);
        return;
    }
    const long long head = ((ax & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;   // tail < n: one element after the last pair
    if (gid == 0 && head) hist_one(s, words, 0, s.x[0]);
    if (gid == 1 && tail < n) hist_one(s, words, tail, s.x[tail]);
    const GD2* __restrict__ x2 = (const GD2*)(s.x + head);
    for (long long p = gid; p < npair; p += stride) {
        const dbl2 x = x2[p];
        hist_one(s, words, head + 2 * p, x.x);
        hist_one(s, words, head + 2 * p + 1, x.y);
    }
}

typedef const SigSeg __attribute__((address_space(4))) * sig_kptr;   // the segment table through the scalar cache (dx_sed.h: kptr)

// comp_sed for a registered signal.  Registration refuses the global-amplitude types, and the host puts a segment into the
// launch of k_moments_signal<false> only when every band of it is a delta bandpass: told so, the compiler drops the template
// and bandpass-integrated forms from the streaming kernel.  The expressions evaluated are comp_sed's in both kernels.
template <bool BP>
__device__ __forceinline__ double sig_sed(const Model& M, const Comp& c, int i, int k, int j, const Prep& p) {
    __builtin_assume(c.type >= DANGX_POWERLAW && c.type <= DANGX_TCMB);
    if (!BP) __builtin_assume(M.band[j].n == 0);
    return comp_sed(M, c, i, k, j, p);
}

// v[e] of four values for a wave-uniform e: explicit selects, so that the register arrays below are never indexed dynamically
__device__ __forceinline__ double sel4(int e, double v0, double v1, double v2, double v3) {
    return e == 0 ? v0 : e == 1 ? v1 : e == 2 ? v2 : v3;
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }   // a wave-uniform value kept in a VGPR
__device__ __forceinline__ void put4(int e, double (&v)[4], double x) {
    v[0] = e == 0 ? x : v[0]; v[1] = e == 1 ? x : v[1]; v[2] = e == 2 ? x : v[2]; v[3] = e == 3 ? x : v[3];
}

// blockIdx.y = segment.  One sample of every registered signal: Welford's update of k_moments_accum on x = eval_signal.
// The blocks of a segment stride over its items: pairs of pixels (16-byte accesses) where every plane read and every accumulator
// share their 16-byte phase (vec), the odd first / last element alone; element by element otherwise.  An item holds up to four
// evaluation slots e = 2 * (plane of the class) + (half of the pair); every slot goes through the SAME code (the loops over e:
// one copy of sed_prep and comp_sed in the kernel), so a result does not depend on which kind of item held its pixel.
template <bool BP>
__global__ __launch_bounds__(BLOCK) void k_moments_signal(const Model* __restrict__ Mp, const SigSeg* __restrict__ segs, double inv_n) {
    const Model& M = *Mp;
    const sig_kptr s = reinterpret_cast<sig_kptr>(reinterpret_cast<uintptr_t>(segs + blockIdx.y));
    const Comp& c = M.comp[s->comp];
    const long long n = s->n;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const int vec = BP ? 0 : s->vec;   // segments with an integrated band: issue bound, element by element
    const long long head = (vec == 2 && n > 0) ? 1 : 0;
    const long long npair = vec ? (n - head) / 2 : 0, tail = head + 2 * npair;   // tail < n: one element after the last pair
    const long long nitems = vec ? npair + head + (tail < n ? 1 : 0) : n;
    // The scalar register file belongs to the SED's band constants (comp_sed alone takes ~95 SGPRs): everything wave-uniform of this
    // kernel's own is parked in vector registers -- the segment's pointers, counts and the band records are read with vector loads
    // through sv -- and comes back through uni() for the few uses that need a scalar (loop bounds, the band index).
    int k0 = s->k0, np2 = 2 * s->np, nb = s->nb, nind = s->nind, estep = vec ? 1 : 2;   // estep: the odd slots of an element-by-element item are not evaluated
    long long item_stride = stride, item_end = nitems, pair_end = npair, i_head = head, i_tail = tail;
    const double *pa0 = s->src[0][0], *pt00 = s->src[0][1], *pt01 = s->src[0][2];
    const double *pa1 = s->src[1][0], *pt10 = s->src[1][1], *pt11 = s->src[1][2];
    const SigBand* sv = segs[blockIdx.y].b;
    asm volatile("" : "+v"(item_stride), "+v"(item_end), "+v"(pair_end), "+v"(i_head), "+v"(i_tail), "+v"(inv_n));
    asm volatile("" : "+v"(pa0), "+v"(pt00), "+v"(pt01), "+v"(pa1), "+v"(pt10), "+v"(pt11), "+v"(sv));
    asm volatile("" : "+v"(k0), "+v"(np2), "+v"(nb), "+v"(nind), "+v"(estep));
    for (long long t = gid; t < item_end; t += item_stride) {
        const bool single = t >= pair_end;
        const long long i = !single ? i_head + 2 * t : !vec ? t : (t == pair_end && i_head) ? 0 : i_tail;   // the item's first pixel
        double a[4] = {0.0, 0.0, 0.0, 0.0}, t0[4] = {0.0, 0.0, 0.0, 0.0}, t1[4] = {0.0, 0.0, 0.0, 0.0};
        if (single) {
            a[0] = pa0[i]; t0[0] = pt00[i]; t1[0] = pt01[i];
            if (np2 == 4) { a[2] = pa1[i]; t0[2] = pt10[i]; t1[2] = pt11[i]; }
        } else {
            dbl2 v = *(const GD2*)(pa0 + i); a[0] = v.x; a[1] = v.y;
            v = *(const GD2*)(pt00 + i); t0[0] = v.x; t0[1] = v.y;
            v = *(const GD2*)(pt01 + i); t1[0] = v.x; t1[1] = v.y;
            if (np2 == 4) {
                v = *(const GD2*)(pa1 + i); a[2] = v.x; a[3] = v.y;
                v = *(const GD2*)(pt10 + i); t0[2] = v.x; t0[3] = v.y;
                v = *(const GD2*)(pt11 + i); t1[2] = v.x; t1[3] = v.y;
            }
        }
        double q0[4] = {0.0, 0.0, 0.0, 0.0}, q1[4] = {0.0, 0.0, 0.0, 0.0}, q2[4] = {0.0, 0.0, 0.0, 0.0};   // the slots' Prep
#pragma nounroll
        for (int e = 0; e < uni(np2); e += uni(estep)) {
            // load_theta's values: an index the component does not have is 0.0 (its slot was loaded from a plane that is read anyway)
            const Prep pr = sed_prep(c, nind > 0 ? sel4(e, t0[0], t0[1], t0[2], t0[3]) : 0.0, nind > 1 ? sel4(e, t1[0], t1[1], t1[2], t1[3]) : 0.0);
            put4(e, q0, pr.p0); put4(e, q1, pr.p1); put4(e, q2, pr.p2);
        }
        for (int b = 0; b < uni(nb); ++b) {
            const unsigned want = sv[b].want;
            const int band = uni(sv[b].band);
            const unsigned planes = (want & 4u) ? 3u : want & 3u;   // P needs both
            double x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma nounroll
            for (int e = 0; e < uni(np2); e += uni(estep)) {
                if (!uni((int)((planes >> (e >> 1)) & 1u))) continue;
                const Prep pr = {sel4(e, q0[0], q0[1], q0[2], q0[3]), sel4(e, q1[0], q1[1], q1[2], q1[3]), sel4(e, q2[0], q2[1], q2[2], q2[3])};
                const double sed = sig_sed<BP>(M, c, (int)i + (single ? 0 : (e & 1)), uni(k0) + (e >> 1), band, pr);   // never a pixel past the item
                // eval_signal: the bare SED for T_cmb, else the ROUNDED product amplitude * sed
                put4(e, x, (c.type == DANGX_TCMB) ? sed : dx_signal_product(sel4(e, a[0], a[1], a[2], a[3]), sed));
            }
            double pol[2] = {0.0, 0.0};
            if (want & 4u) {
                pol[0] = dx_signal_pol(x[0], x[2]);
                pol[1] = dx_signal_pol(x[1], x[3]);
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                if (!((want >> o) & 1u)) continue;
                const double y0 = o == 0 ? x[0] : o == 1 ? x[2] : pol[0], y1 = o == 0 ? x[1] : o == 1 ? x[3] : pol[1];
                double* mp = sv[b].mean[o] + i;
                double* qp = sv[b].m2[o] + i;
                if (single) {
                    double m = *mp, q = *qp;
                    welford(y0, m, q, inv_n);
                    *mp = m; *qp = q;
                } else {
                    const dbl2 m = *(GD2*)mp, q = *(GD2*)qp;
                    double m0 = m.x, m1 = m.y, r0 = q.x, r1 = q.y;
                    welford(y0, m0, r0, inv_n);
                    welford(y1, m1, r1, inv_n);
                    *(GD2*)mp = dbl2{m0, m1}; *(GD2*)qp = dbl2{r0, r1};
                }
            }
        }
    }
}

struct HistStatArgs {
    const uint32_t* rec;
    double q[DX_HIST_MAX_Q];   // the quantile levels (stat 0), by value: nothing of the caller's is read after the call returns
    double* out;          // [nq][n] (stat 0) or [n]
    double lo, hi;
    long long n;
    int nbins, bits, stat, nq;
};

// every 16-byte piece of pixel i's record in order, f(count, bin) per bin until f says stop
template <class F>
__device__ __forceinline__ void hist_walk(const GU4* __restrict__ rec, long long i, int pieces, int bits, F f) {
    int b = 0;
    for (int p = 0; p < pieces; ++p) {
        const u32x4 v = rec[i * pieces + p];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (bits == 16) {
                if (f(w[k] & 0xffffu, b)) return;
                if (f(w[k] >> 16, b + 1)) return;
                b += 2;
            } else {
                if (f(w[k], b)) return;
                ++b;
            }
        }
    }
}

// a lane walks its own record: once for N and the mode, once more per quantile (those passes hit the cache)
__global__ __launch_bounds__(BLOCK) void k_hist_stat(HistStatArgs a) {
    const GU4* __restrict__ rec = (const GU4*)a.rec;
    const int pieces = dx_hist_words(a.nbins, a.bits) / 4;
    const double width = (a.hi - a.lo) / (double)a.nbins;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
        unsigned long long N = 0;
        uint32_t best_c = 0;
        int best_b = -1;
        hist_walk(rec, i, pieces, a.bits, [&](uint32_t c, int b) { N += c; dx_hist_mstep(c, b, best_c, best_b); return false; });
        if (a.stat == 1) { a.out[i] = dx_hist_mode_value(best_b, a.lo, width); continue; }
        if (a.stat == 2) { a.out[i] = (double)N; continue; }
        for (int j = 0; j < a.nq; ++j) {
            double val = (double)NAN;
            if (N > 0) {
                const double target = a.q[j] * (double)N;
                unsigned long long cum = 0;
                hist_walk(rec, i, pieces, a.bits, [&](uint32_t c, int b) { return dx_hist_qstep(c, b, target, cum, a.lo, width, val); });
            }
            a.out[(long long)j * a.n + i] = val;
        }
    }
}

struct FinishLagArgs {
    const double* mean[3];
    const double* m2[3];
    const double* prev[3];
    const double* first[3];
    const double* P[3];
    double* out[3];
    long long n;
    int stat;    // 2 = rho1, 3 = ESS
    double cnt;  // samples
};

__global__ __launch_bounds__(BLOCK) void k_moments_finish_lag(FinishLagArgs a) {
    const int p = blockIdx.y;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
        const double rho = dx_lag_rho1(a.mean[p][i], a.m2[p][i], a.prev[p][i], a.first[p][i], a.P[p][i], a.cnt);
        a.out[p][i] = a.stat == 2 ? rho : dx_lag_ess(rho, a.cnt);
    }
}

// out = C / (n - ddof), or C / sqrt(m2_a m2_b)
__global__ __launch_bounds__(BLOCK) void k_moments_finish_pair(const double* __restrict__ C, const double* __restrict__ m2a,
                                                               const double* __restrict__ m2b, double* __restrict__ out, long long n,
                                                               int stat, double dn) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK)
        out[i] = dx_pair_stat(C[i], m2a[i], m2b[i], stat, dn);
}

struct FinishArgs {
    const double* mean[3];
    const double* m2[3];
    double* out[3];
    long long n;
    int stat;
    double dn;   // n - ddof
};

// blockIdx.y = plane: out = mean, or sqrt(m2 / (n - ddof))
__global__ __launch_bounds__(BLOCK) void k_moments_finish(FinishArgs a) {
    const int p = blockIdx.y;
    const double* __restrict__ mean = a.mean[p];
    const double* __restrict__ m2 = a.m2[p];
    double* __restrict__ out = a.out[p];
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK)
        out[i] = a.stat == 0 ? mean[i] : sqrt(m2[i] / a.dn);
}

void host_welford(double x, double& mean, double& m2, double inv_n) {
    const double d = x - mean;
    mean = std::fma(d, inv_n, mean);
    m2 = std::fma(d, x - mean, m2);
}

int sel_bits(const dangx_ctx* ctx, int comp) {   // every plane the component has
    if (is_global_type(ctx->desc[comp].type)) return (1 << ctx->dims.nmaps) - 1;
    int b = (1 << ctx->dims.nmaps) - 1;
    for (int j = 0; j < ctx->desc[comp].nindices; ++j) b |= ((1 << ctx->dims.nmaps) - 1) << (3 + 3 * j);
    return b;
}

int need(dangx_ctx* ctx) {
    if (!ctx->mom) return fail(ctx, "posterior moments: dangx_moments_begin was not called");
    return 0;
}

void release(DxMoments* m) {
    if (!m) return;
    if (m->d_table) (void)hipFree(m->d_table);
    if (m->acc) (void)hipFree(m->acc);
    if (m->scratch) (void)hipFree(m->scratch);
    if (m->lag) (void)hipFree(m->lag);
    if (m->d_lag) (void)hipFree(m->d_lag);
    if (m->pc) (void)hipFree(m->pc);
    if (m->d_pairs) (void)hipFree(m->d_pairs);
    if (m->hrec) (void)hipFree(m->hrec);
    if (m->d_hist) (void)hipFree(m->d_hist);
    if (m->hscratch) (void)hipFree(m->hscratch);
    if (m->d_sig) (void)hipFree(m->d_sig);
    if (m->sacc) (void)hipFree(m->sacc);
    if (m->chain_ev) (void)hipEventDestroy(m->chain_ev);
    delete m;
}

// the resident plane of a segment as it is now (adopted buffers may have been replaced since begin)
const double* seg_plane(const dangx_ctx* ctx, const DxMoments::Seg& s) {
    const long long np = ctx->dims.npix;
    if (s.what == 0) return ctx->amp[s.comp] + (long long)s.plane * np;
    return ctx->idx[s.comp] + ((long long)(s.what - 1) * ctx->dims.nmaps + s.plane) * np;
}

// checks of a get: planes of (comp, what) that are selected -> bit k = plane k+1
int get_planes(dangx_ctx* ctx, int comp, int what, int stat, int ddof, unsigned& planes) {
    if (need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    if (comp < 0 || comp >= ctx->dims.ncomp) return fail(ctx, "posterior moments: component index out of range");
    if (what < 0 || what > DANGX_MAX_IND) return fail(ctx, "posterior moments: what must be 0 (amplitude) or 1 + index number");
    if (stat < 0 || stat > 3)
        return fail(ctx, "posterior moments: stat must be 0 (mean), 1 (standard deviation), 2 (lag-1 autocorrelation) or 3 (effective sample size)");
    if (stat >= 2 && !m->lag1)
        return fail(ctx, "posterior moments: the lag-1 autocorrelation is not tracked (dangx_moments_pairs with lag1 != 0 was not called)");
    if (m->count == 0) return fail(ctx, "posterior moments: no sample accumulated");
    if (stat == 1 && (ddof < 0 || m->count - ddof <= 0)) return fail(ctx, "posterior moments: standard deviation needs 0 <= ddof < n");
    planes = (unsigned)(m->sel[comp] >> (what == 0 ? 0 : 3 + 3 * (what - 1))) & 7u;
    if (!planes) return fail(ctx, "posterior moments: nothing selected for this component and what");
    return 0;
}

// k_moments_finish of the selected planes of (comp, what) into dst ([nmaps][npix], device)
int finish(dangx_ctx* ctx, int comp, int what, int stat, int ddof, unsigned planes, double* dst) {
    DxMoments* m = ctx->mom;
    if (stat >= 2) {   // rho1 / ESS from the lag-1 state
        FinishLagArgs a{};
        int np = 0;
        for (const auto& s : m->segs) {
            if (s.comp != comp || s.what != what || !((planes >> s.plane) & 1u)) continue;
            a.mean[np] = m->acc + s.off;
            a.m2[np] = m->acc + m->acc_half + s.off;
            a.prev[np] = m->lag + s.off;
            a.first[np] = m->lag + m->acc_half + s.off;
            a.P[np] = m->lag + 2 * m->acc_half + s.off;
            a.out[np] = dst + (long long)s.plane * ctx->dims.npix;
            ++np;
        }
        a.n = ctx->dims.npix;
        a.stat = stat;
        a.cnt = (double)m->count;
        const unsigned gx = std::max(1u, std::min(nblocks(a.n), 1024u));
        hipLaunchKernelGGL(k_moments_finish_lag, dim3(gx, np), dim3(BLOCK), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
        return 0;
    }
    FinishArgs a{};
    int np = 0;
    for (const auto& s : m->segs) {
        if (s.comp != comp || s.what != what || !((planes >> s.plane) & 1u)) continue;
        a.mean[np] = m->acc + s.off;
        a.m2[np] = m->acc + m->acc_half + s.off;
        a.out[np] = dst + (long long)s.plane * ctx->dims.npix;
        ++np;
    }
    a.n = ctx->dims.npix;
    a.stat = stat;
    a.dn = (double)(m->count - ddof);
    const unsigned gx = std::max(1u, std::min(nblocks(a.n), 1024u));
    hipLaunchKernelGGL(k_moments_finish, dim3(gx, np), dim3(BLOCK), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// first plane (1-based) and plane count of a class
inline int sig_k0(int cls) { return cls == 0 ? 1 : 2; }

// the device table of the registered signals for the chain's planes as they are now
size_t sig_table(const dangx_ctx* ctx, const DxMoments* m, std::vector<SigSeg>& t) {
    const long long np = ctx->dims.npix;
    const int nmaps = ctx->dims.nmaps;
    t.clear();
    size_t ndelta = 0;   // delta-band segments first (k_moments_signal<false>), then those with an integrated band
    for (int pass = 0; pass < 2; ++pass)
    for (const DxSigSeg& ps : m->sig_plan) {
        bool bp = false;
        for (int b = 0; b < ps.nb; ++b) bp = bp || ctx->hm.band[ps.b[b].band].n != 0;
        if (bp != (pass == 1)) continue;
        if (!bp) ++ndelta;
        SigSeg s;
        std::memset(&s, 0, sizeof s);   // the tables are compared as bytes
        s.amp = ctx->amp[ps.comp];
        s.idx = ctx->idx[ps.comp];
        s.n = np;
        s.comp = ps.comp; s.k0 = sig_k0(ps.cls); s.np = ps.cls == 0 ? 1 : 2; s.nb = ps.nb;
        s.nind = ctx->desc[ps.comp].nindices;
        uintptr_t phase = 0, diff = 0;   // diff: bit 3 set when two addresses differ in their 16-byte phase
        bool first = true;
        auto see = [&](const double* q) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(q);
            if (first) { phase = a; first = false; }
            diff |= (a ^ phase) & 15;
        };
        unsigned needp = 0;              // bit k: an output of some band needs plane k0 + k
        for (int b = 0; b < ps.nb; ++b) {
            SigBand& sb = s.b[b];
            sb.band = ps.b[b].band;
            for (int o = 0; o < 3; ++o) {
                const int sg = ps.b[b].sig[o];
                if (sg < 0) continue;
                sb.want |= 1u << o;
                sb.mean[o] = m->sacc + m->sigs[sg].off;
                sb.m2[o] = m->sacc + m->sacc_half + m->sigs[sg].off;
                see(sb.mean[o]); see(sb.m2[o]);
                needp |= (o == 2) ? 3u : 1u << o;
            }
        }
        const double* fallback = s.amp + (long long)(s.k0 - 1 + ((needp & 1u) ? 0 : 1)) * np;   // an amplitude plane that is read
        for (int k = 0; k < 2; ++k) {
            const long long plane = s.k0 - 1 + k;
            const bool read = k < s.np && ((needp >> k) & 1u);
            for (int q = 0; q < 3; ++q) {
                const bool has = read && (q == 0 || q - 1 < ctx->desc[ps.comp].nindices);
                s.src[k][q] = !has ? fallback : q == 0 ? s.amp + plane * np : s.idx + ((long long)(q - 1) * nmaps + plane) * np;
                see(s.src[k][q]);
            }
        }
        s.vec = diff ? 0 : ((phase & 15) ? 2 : 1);
        t.push_back(s);
    }
    return ndelta;
}

// finish of one plane pair (mean, m2) into dst [npix]
int finish_plane(dangx_ctx* ctx, const double* mean, const double* m2, int stat, double dn, double* dst) {
    FinishArgs a{};
    a.mean[0] = mean; a.m2[0] = m2; a.out[0] = dst;
    a.n = ctx->dims.npix;
    a.stat = stat;
    a.dn = dn;
    const unsigned gx = std::max(1u, std::min(nblocks(a.n), 1024u));
    hipLaunchKernelGGL(k_moments_finish, dim3(gx, 1), dim3(BLOCK), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int signal_get_check(dangx_ctx* ctx, int sig, int stat, int ddof) {
    if (need(ctx)) return 1;
    const DxMoments* m = ctx->mom;
    if (sig < 0 || sig >= (int)m->sigs.size())
        return fail(ctx, "posterior moments: signal index out of range (" + std::to_string(m->sigs.size()) + " signals registered)");
    if (stat != 0 && stat != 1) return fail(ctx, "posterior moments: the stat of a signal must be 0 (mean) or 1 (standard deviation)");
    if (m->count == 0) return fail(ctx, "posterior moments: no sample accumulated");
    if (stat == 1 && (ddof < 0 || m->count - ddof <= 0)) return fail(ctx, "posterior moments: standard deviation needs 0 <= ddof < n");
    return 0;
}

}  // namespace

void dx_moments_free(dangx_ctx* ctx) {
    release(ctx->mom);
    ctx->mom = nullptr;
}

extern "C" {

int dangx_moments_begin(dangx_ctx* ctx, const int32_t* sel) {
    if (!ctx) return 1;
    (void)hipSetDevice(ctx->device);
    const int ncomp = ctx->dims.ncomp, nmaps = ctx->dims.nmaps;
    int32_t eff[MAXC] = {};
    for (int l = 0; l < ncomp; ++l) {
        if (!sel) { eff[l] = ctx->comp_set[l] ? sel_bits(ctx, l) : 0; continue; }
        if (!sel[l]) continue;
        if (!ctx->comp_set[l]) return fail(ctx, "posterior moments: a selected component is not set");
        if (sel[l] & ~sel_bits(ctx, l))
            return fail(ctx, "posterior moments: the selection of component " + std::to_string(l) + " names planes it does not have");
        eff[l] = sel[l];
    }
    for (int l = 0; l < ncomp; ++l)   // the chain's maps exist from here on (what dangx_get_amplitude does on first use)
        if (eff[l] && !is_global_type(ctx->desc[l].type) && ensure_state(ctx, l)) return 1;
    DxMoments* m = new DxMoments();
    for (int l = 0; l < ncomp; ++l) {
        m->sel[l] = eff[l];
        m->type[l] = ctx->desc[l].type;
        m->nind[l] = ctx->desc[l].nindices;
    }
    // accumulators: every plane at the 16-byte phase of the chain's plane, so that the three streams line up
    long long off = 0;
    for (int l = 0; l < ncomp; ++l) {
        if (is_global_type(ctx->desc[l].type)) continue;
        for (int w = 0; w <= ctx->desc[l].nindices; ++w)
            for (int k = 0; k < nmaps; ++k) {
                if (!((eff[l] >> (w == 0 ? k : 3 + 3 * (w - 1) + k)) & 1)) continue;
                DxMoments::Seg s{l, w, k, 0};
                const long long phase = (long long)((reinterpret_cast<uintptr_t>(seg_plane(ctx, s)) >> 3) & 1);
                if ((off & 1) != phase) ++off;
                s.off = off;
                off += ctx->dims.npix;
                m->segs.push_back(s);
            }
    }
    m->acc_half = off + (off & 1);   // even: the m2 half has the phases of the mean half
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || ncu <= 0) ncu = 256;
    m->grid_target = 8u * (unsigned)ncu;
    auto bail = [&](hipError_t e, const char* what) {
        ctx->err = std::string("posterior moments: ") + what + ": " + hipGetErrorString(e);
        release(m);
        return 1;
    };
    hipError_t e;
    if (!m->segs.empty()) {
        if ((e = hipMalloc(&m->acc, sizeof(double) * 2 * (size_t)m->acc_half)) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipMemsetAsync(m->acc, 0, sizeof(double) * 2 * (size_t)m->acc_half, ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
        if ((e = hipMalloc(&m->d_table, sizeof(MomSeg) * m->segs.size())) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    }
    dx_moments_free(ctx);   // calling begin again starts over
    ctx->mom = m;
    return 0;
}

int dangx_moments_pairs(dangx_ctx* ctx, int lag1, int npairs, const int32_t* pairs) {
    if (!ctx || need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    if (m->count != 0)
        return fail(ctx, "posterior moments: dangx_moments_pairs is legal only before the first dangx_moments_accumulate after dangx_moments_begin");
    const int ncomp = ctx->dims.ncomp;
    int nind[MAXC] = {}, global[MAXC] = {};
    for (int l = 0; l < ncomp; ++l) {
        nind[l] = m->nind[l];
        global[l] = is_global_type(m->type[l]) ? 1 : 0;
    }
    const std::string why = dx_pairs_check(npairs, pairs, ncomp, ctx->dims.nmaps, m->sel, nind, global);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_pairs: " + why);
    auto seg_of = [&](const int32_t* q) {
        for (size_t i = 0; i < m->segs.size(); ++i)
            if (m->segs[i].comp == q[0] && m->segs[i].what == q[1] && m->segs[i].plane == q[2]) return (int)i;
        return -1;
    };
    std::vector<DxMoments::Pair> np;
    long long off = 0;
    for (int p = 0; p < npairs; ++p) {
        DxMoments::Pair pr{seg_of(pairs + 6 * p), seg_of(pairs + 6 * p + 3), 0};
        if (pr.a < 0 || pr.b < 0) return fail(ctx, "posterior moments: dangx_moments_pairs: pair " + std::to_string(p) + ": a plane that is not selected");
        if ((off & 1) != (m->segs[pr.a].off & 1)) ++off;
        pr.off = off;
        off += ctx->dims.npix;
        np.push_back(pr);
    }
    (void)hipSetDevice(ctx->device);
    // everything new is allocated before anything old is dropped: a failure leaves the registration as it was
    double *lag = nullptr, *pc = nullptr;
    LagSeg* d_lag = nullptr;
    PairSeg* d_pairs = nullptr;
    auto bail = [&](hipError_t e, const char* what) {
        ctx->err = std::string("posterior moments: dangx_moments_pairs: ") + what + ": " + hipGetErrorString(e);
        if (lag) (void)hipFree(lag);
        if (pc) (void)hipFree(pc);
        if (d_lag) (void)hipFree(d_lag);
        if (d_pairs) (void)hipFree(d_pairs);
        return 1;
    };
    hipError_t e;
    if (lag1 && !m->segs.empty()) {
        const size_t bytes = sizeof(double) * 3 * (size_t)m->acc_half;
        if ((e = hipMalloc(&lag, bytes)) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipMemsetAsync(lag, 0, bytes, ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
        if ((e = hipMalloc(&d_lag, sizeof(LagSeg) * m->segs.size())) != hipSuccess) return bail(e, "hipMalloc");
    }
    if (!np.empty()) {
        if ((e = hipMalloc(&pc, sizeof(double) * (size_t)off)) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipMemsetAsync(pc, 0, sizeof(double) * (size_t)off, ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
        if ((e = hipMalloc(&d_pairs, sizeof(PairSeg) * np.size())) != hipSuccess) return bail(e, "hipMalloc");
    }
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    if (m->lag) (void)hipFree(m->lag);
    if (m->d_lag) (void)hipFree(m->d_lag);
    if (m->pc) (void)hipFree(m->pc);
    if (m->d_pairs) (void)hipFree(m->d_pairs);
    m->lag = lag; m->d_lag = d_lag; m->pc = pc; m->d_pairs = d_pairs;
    m->lag1 = lag1 != 0;
    m->pairs = np;
    m->table.clear();   // the next accumulation uploads the tables
    std::memset(m->tm_prev, 0, sizeof m->tm_prev);
    std::memset(m->tm_first, 0, sizeof m->tm_first);
    std::memset(m->tm_P, 0, sizeof m->tm_P);
    return 0;
}

int dangx_moments_accumulate(dangx_ctx* ctx) {
    if (!ctx || need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    for (int l = 0; l < ctx->dims.ncomp; ++l)
        if (m->sel[l] && (!ctx->comp_set[l] || ctx->desc[l].type != m->type[l] || ctx->desc[l].nindices != m->nind[l]))
            return fail(ctx, "posterior moments: component " + std::to_string(l) + " changed type or nindices since dangx_moments_begin");
    for (int l = 0; l < ctx->dims.ncomp; ++l)
        if (m->sig_used[l] && (!ctx->comp_set[l] || ctx->desc[l].type != m->sig_type[l] || ctx->desc[l].nindices != m->sig_nind[l]))
            return fail(ctx, "posterior moments: component " + std::to_string(l) + " changed type or nindices since dangx_moments_signals");
    if (ctx->have_pending) return fail(ctx, "posterior moments: an amplitude solve is still pending");   // not at a call boundary
    if (!m->hists.empty()) {   // no counter ever wraps: refused before anything is touched
        const std::string why = dx_hist_limit_check(m->count + 1, m->hbits);
        if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_accumulate: " + why);
    }
    (void)hipSetDevice(ctx->device);
    if (!m->sigs.empty() && sync_model(ctx)) return 1;   // the SEDs read the device model: current before anything is launched
    const double inv_n = 1.0 / (double)(m->count + 1);
    if (!m->segs.empty()) {
        std::vector<MomSeg> t(m->segs.size());
        for (size_t i = 0; i < t.size(); ++i) {
            const auto& s = m->segs[i];
            t[i] = MomSeg{seg_plane(ctx, s), m->acc + s.off, m->acc + m->acc_half + s.off, (long long)ctx->dims.npix};
        }
        bool same = t.size() == m->table.size();
        for (size_t i = 0; same && i < t.size(); ++i) same = t[i].x == m->table[i].x;
        if (!same) {   // first accumulation, or a component's buffers were adopted again: one upload (and a host wait) here only
            HIPCHK(ctx, hipMemcpyAsync(m->d_table, t.data(), sizeof(MomSeg) * t.size(), hipMemcpyHostToDevice, ctx->stream));
            std::vector<LagSeg> tl;
            std::vector<PairSeg> tp;
            if (m->d_lag) {
                for (size_t i = 0; i < t.size(); ++i) {
                    double* g = m->lag + m->segs[i].off;
                    tl.push_back(LagSeg{t[i].x, t[i].mean, t[i].m2, g, g + m->acc_half, g + 2 * m->acc_half, t[i].n});
                }
                HIPCHK(ctx, hipMemcpyAsync(m->d_lag, tl.data(), sizeof(LagSeg) * tl.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            if (m->d_pairs) {
                for (const auto& p : m->pairs)
                    tp.push_back(PairSeg{t[p.a].x, t[p.b].x, t[p.a].mean, t[p.b].mean, m->pc + p.off, (long long)ctx->dims.npix});
                HIPCHK(ctx, hipMemcpyAsync(m->d_pairs, tp.data(), sizeof(PairSeg) * tp.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            std::vector<HistSeg> th;
            if (m->d_hist) {
                for (const auto& h : m->hists)
                    th.push_back(HistSeg{t[h.seg].x, m->hrec + h.off, h.lo, h.hi, dx_hist_scale(h.lo, h.hi, m->hbins), (long long)ctx->dims.npix,
                                         m->hbins, m->hbits});
                HIPCHK(ctx, hipMemcpyAsync(m->d_hist, th.data(), sizeof(HistSeg) * th.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            m->table = t;
        }
        const long long pairs = (ctx->dims.npix + 1) / 2;
        if (!m->pairs.empty()) {   // the cross terms read the means of the previous accumulation: a launch of its own, first
            const unsigned npr = (unsigned)m->pairs.size();
            const unsigned gx = std::max(1u, std::min(nblocks(pairs), (m->grid_target + npr - 1) / npr));
            Timed tm(ctx, DANGX_K_MOMENTS, 2);   // the profile tells them apart by their plane count: two planes per element
            hipLaunchKernelGGL(k_moments_pairs, dim3(gx, npr), dim3(BLOCK), 0, ctx->stream, (const PairSeg*)m->d_pairs, inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
        const unsigned nseg = (unsigned)t.size();
        const unsigned gx = std::max(1u, std::min(nblocks(pairs), (m->grid_target + nseg - 1) / nseg));
        Timed tm(ctx, DANGX_K_MOMENTS);
        if (!m->lag1)
            hipLaunchKernelGGL(k_moments_accum, dim3(gx, nseg), dim3(BLOCK), 0, ctx->stream, (const MomSeg*)m->d_table, inv_n);
        else if (m->count == 0)
            hipLaunchKernelGGL(k_moments_accum_lag<true>, dim3(gx, nseg), dim3(BLOCK), 0, ctx->stream, (const LagSeg*)m->d_lag, inv_n);
        else
            hipLaunchKernelGGL(k_moments_accum_lag<false>, dim3(gx, nseg), dim3(BLOCK), 0, ctx->stream, (const LagSeg*)m->d_lag, inv_n);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!m->hists.empty()) {   // the histograms: a launch of their own, independent of the accumulators above
        const long long pairs = (ctx->dims.npix + 1) / 2;
        const unsigned nreg = (unsigned)m->hists.size();
        const unsigned gx = std::max(1u, std::min(nblocks(pairs), (m->grid_target + nreg - 1) / nreg));
        Timed tm(ctx, DANGX_K_HIST);
        hipLaunchKernelGGL(k_moments_hist, dim3(gx, nreg), dim3(BLOCK), 0, ctx->stream, (const HistSeg*)m->d_hist);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!m->sigs.empty()) {   // the component signals: a launch of their own, independent of everything above
        std::vector<SigSeg> t;
        const size_t ndelta = sig_table(ctx, m, t);
        const bool same = t.size() == m->sig_table.size() && std::memcmp(t.data(), m->sig_table.data(), sizeof(SigSeg) * t.size()) == 0;
        if (!same) {   // first accumulation, a component's buffers adopted again or a band's bandpass replaced: one upload (and a host wait)
            HIPCHK(ctx, hipMemcpyAsync(m->d_sig, t.data(), sizeof(SigSeg) * t.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            m->sig_table = t;
        }
        const long long pairs = (ctx->dims.npix + 1) / 2;
        if (ndelta) {
            const unsigned nseg = (unsigned)ndelta;
            const unsigned gx = std::max(1u, std::min(nblocks(pairs), (m->grid_target + nseg - 1) / nseg));
            Timed tm(ctx, DANGX_K_SIGNAL);
            hipLaunchKernelGGL(k_moments_signal<false>, dim3(gx, nseg), dim3(BLOCK), 0, ctx->stream, (const Model*)ctx->dm,
                               (const SigSeg*)m->d_sig, inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
        if (t.size() > ndelta) {   // segments with an integrated band: element by element
            const unsigned nseg = (unsigned)(t.size() - ndelta);
            const unsigned gx = std::max(1u, std::min(nblocks(ctx->dims.npix), (m->grid_target + nseg - 1) / nseg));
            Timed tm(ctx, DANGX_K_SIGNAL, 2);   // the profile tells the two forms apart by this mark
            hipLaunchKernelGGL(k_moments_signal<true>, dim3(gx, nseg), dim3(BLOCK), 0, ctx->stream, (const Model*)ctx->dm,
                               (const SigSeg*)(m->d_sig + ndelta), inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    for (int l = 0; l < ctx->dims.ncomp; ++l) {
        if (!m->sel[l] || !is_global_type(ctx->desc[l].type)) continue;
        for (int k = 0; k < ctx->dims.nmaps; ++k)
            if ((m->sel[l] >> k) & 1)
                for (int j = 0; j < ctx->dims.nbands; ++j) {
                    const double x = ctx->tamp[l][k][j];
                    if (m->lag1) {
                        if (m->count == 0) m->tm_prev[l][k][j] = m->tm_first[l][k][j] = x;
                        else dx_lag_update(x, m->tm_prev[l][k][j], m->tm_first[l][k][j], m->tm_P[l][k][j]);
                    }
                    host_welford(x, m->tm_mean[l][k][j], m->tm_m2[l][k][j], inv_n);
                }
    }
    ++m->count;
    return 0;
}

int dangx_moments_count(dangx_ctx* ctx, int64_t* n) {
    if (!ctx || !n || need(ctx)) return 1;
    *n = ctx->mom->count;
    return 0;
}

int dangx_moments_get_dev(dangx_ctx* ctx, int comp, int what, int stat, int ddof, double* out_dev) {
    if (!ctx || !out_dev) return 1;
    unsigned planes = 0;
    if (get_planes(ctx, comp, what, stat, ddof, planes)) return 1;
    if (what == 0 && is_global_type(ctx->desc[comp].type))
        return fail(ctx, "posterior moments: a template / monopole / hi_fit amplitude is read with dangx_moments_get_template");
    (void)hipSetDevice(ctx->device);
    return finish(ctx, comp, what, stat, ddof, planes, out_dev);
}

int dangx_moments_get(dangx_ctx* ctx, int comp, int what, int stat, int ddof, double* out) {
    if (!ctx || !out) return 1;
    unsigned planes = 0;
    if (get_planes(ctx, comp, what, stat, ddof, planes)) return 1;
    if (what == 0 && is_global_type(ctx->desc[comp].type))
        return fail(ctx, "posterior moments: a template / monopole / hi_fit amplitude is read with dangx_moments_get_template");
    (void)hipSetDevice(ctx->device);
    DxMoments* m = ctx->mom;
    const long long np = ctx->dims.npix;
    if (!m->scratch) HIPCHK(ctx, hipMalloc(&m->scratch, sizeof(double) * (size_t)np * ctx->dims.nmaps));
    if (finish(ctx, comp, what, stat, ddof, planes, m->scratch)) return 1;
    const long long hs = ctx->host_stride > 0 ? ctx->host_stride : np;
    for (int k = 0; k < ctx->dims.nmaps; ++k)
        if ((planes >> k) & 1u)
            HIPCHK(ctx, hipMemcpyAsync(out + (long long)k * hs, m->scratch + (long long)k * np, sizeof(double) * (size_t)np,
                                       hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_get_template(dangx_ctx* ctx, int comp, int stat, int ddof, double* ta) {
    if (!ctx || !ta) return 1;
    unsigned planes = 0;
    if (get_planes(ctx, comp, 0, stat, ddof, planes)) return 1;
    if (!is_global_type(ctx->desc[comp].type)) return fail(ctx, "posterior moments: not a template / monopole / hi_fit component");
    const DxMoments* m = ctx->mom;
    const double dn = (double)(m->count - ddof);
    for (int k = 0; k < ctx->dims.nmaps; ++k)
        if ((planes >> k) & 1u)
            for (int j = 0; j < ctx->dims.nbands; ++j) {
                double v;
                if (stat >= 2) {
                    v = dx_lag_rho1(m->tm_mean[comp][k][j], m->tm_m2[comp][k][j], m->tm_prev[comp][k][j], m->tm_first[comp][k][j],
                                    m->tm_P[comp][k][j], (double)m->count);
                    if (stat == 3) v = dx_lag_ess(v, (double)m->count);
                } else {
                    v = stat == 0 ? m->tm_mean[comp][k][j] : std::sqrt(m->tm_m2[comp][k][j] / dn);
                }
                ta[k * ctx->dims.nbands + j] = v;
            }
    return 0;
}

int dangx_moments_get_pair_dev(dangx_ctx* ctx, int pair, int stat, int ddof, double* out_dev) {
    if (!ctx || !out_dev || need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    if (pair < 0 || pair >= (int)m->pairs.size())
        return fail(ctx, "posterior moments: pair index out of range (" + std::to_string(m->pairs.size()) + " pairs registered)");
    if (stat != 0 && stat != 1) return fail(ctx, "posterior moments: the stat of a pair must be 0 (covariance) or 1 (correlation)");
    if (m->count == 0) return fail(ctx, "posterior moments: no sample accumulated");
    if (stat == 0 && (ddof < 0 || m->count - ddof <= 0)) return fail(ctx, "posterior moments: covariance needs 0 <= ddof < n");
    (void)hipSetDevice(ctx->device);
    const auto& p = m->pairs[pair];
    const long long n = ctx->dims.npix;
    const unsigned gx = std::max(1u, std::min(nblocks(n), 1024u));
    hipLaunchKernelGGL(k_moments_finish_pair, dim3(gx), dim3(BLOCK), 0, ctx->stream, (const double*)(m->pc + p.off),
                       (const double*)(m->acc + m->acc_half + m->segs[p.a].off), (const double*)(m->acc + m->acc_half + m->segs[p.b].off),
                       out_dev, n, stat, (double)(m->count - ddof));
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int dangx_moments_get_pair(dangx_ctx* ctx, int pair, int stat, int ddof, double* out) {
    if (!ctx || !out || need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const long long np = ctx->dims.npix;
    if (!m->scratch) HIPCHK(ctx, hipMalloc(&m->scratch, sizeof(double) * (size_t)np * ctx->dims.nmaps));
    if (dangx_moments_get_pair_dev(ctx, pair, stat, ddof, m->scratch)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(out, m->scratch, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_hist(dangx_ctx* ctx, int nreg, const int32_t* planes, const double* range, int nbins, int bits) {
    if (!ctx || need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    if (m->count != 0)
        return fail(ctx, "posterior moments: dangx_moments_hist is legal only before the first dangx_moments_accumulate after dangx_moments_begin");
    const int ncomp = ctx->dims.ncomp;
    int nind[MAXC] = {}, global[MAXC] = {};
    for (int l = 0; l < ncomp; ++l) {
        nind[l] = m->nind[l];
        global[l] = is_global_type(m->type[l]) ? 1 : 0;
    }
    // the ranges with the defaults filled in: an index plane's is that index's uni_prior as the descriptor holds it now
    const int nr = std::max(0, std::min(nreg, DX_HIST_MAX));
    std::vector<double> rg(2 * (size_t)nr, 0.0);
    std::vector<int> has(nr, 0);
    for (int r = 0; planes && r < nr; ++r) {
        const int l = planes[3 * r], w = planes[3 * r + 1];
        if (range && !std::isnan(range[2 * r])) {
            rg[2 * r] = range[2 * r]; rg[2 * r + 1] = range[2 * r + 1];
            has[r] = 1;
        } else if (l >= 0 && l < ncomp && w >= 1 && w <= nind[l] && w <= DANGX_MAX_IND) {
            rg[2 * r] = ctx->desc[l].uni_prior[w - 1][0]; rg[2 * r + 1] = ctx->desc[l].uni_prior[w - 1][1];
            has[r] = 1;
        } else if (w != 0) {
            has[r] = 1;   // out of range: dx_hist_check names it
        }
    }
    const std::string why = dx_hist_check(nreg, planes, rg.data(), has.data(), nbins, bits, ncomp, ctx->dims.nmaps, m->sel, nind, global);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_hist: " + why);
    const long long np = ctx->dims.npix, words = dx_hist_words(nbins, bits);
    std::vector<DxMoments::Hist> nh;
    long long off = 0;   // in 32-bit words; every registration's block starts at a multiple of 256 bytes
    for (int r = 0; r < nreg; ++r) {
        int seg = -1;
        for (size_t i = 0; i < m->segs.size(); ++i)
            if (m->segs[i].comp == planes[3 * r] && m->segs[i].what == planes[3 * r + 1] && m->segs[i].plane == planes[3 * r + 2]) seg = (int)i;
        if (seg < 0) return fail(ctx, "posterior moments: dangx_moments_hist: registration " + std::to_string(r) + ": a plane that is not selected");
        nh.push_back(DxMoments::Hist{seg, rg[2 * r], rg[2 * r + 1], off});
        off += (np * words + 63) / 64 * 64;
    }
    (void)hipSetDevice(ctx->device);
    // everything new is allocated before anything old is dropped: a failure leaves the registration as it was
    uint32_t* hrec = nullptr;
    HistSeg* d_hist = nullptr;
    auto bail = [&](hipError_t e, const char* what) {
        ctx->err = std::string("posterior moments: dangx_moments_hist: ") + what + ": " + hipGetErrorString(e);
        if (hrec) (void)hipFree(hrec);
        if (d_hist) (void)hipFree(d_hist);
        return 1;
    };
    hipError_t e;
    if (!nh.empty()) {
        if ((e = hipMalloc(&hrec, sizeof(uint32_t) * (size_t)off)) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipMemsetAsync(hrec, 0, sizeof(uint32_t) * (size_t)off, ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
        if ((e = hipMalloc(&d_hist, sizeof(HistSeg) * nh.size())) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    }
    if (m->hrec) (void)hipFree(m->hrec);
    if (m->d_hist) (void)hipFree(m->d_hist);
    m->hrec = hrec; m->d_hist = d_hist;
    m->hists = nh;
    m->hbins = nbins; m->hbits = bits;
    m->table.clear();   // the next accumulation uploads the tables
    return 0;
}

namespace {

int hist_reg(dangx_ctx* ctx, int reg) {
    if (need(ctx)) return 1;
    const DxMoments* m = ctx->mom;
    if (reg < 0 || reg >= (int)m->hists.size())
        return fail(ctx, "posterior moments: histogram registration out of range (" + std::to_string(m->hists.size()) + " registered)");
    if (m->count == 0) return fail(ctx, "posterior moments: no sample accumulated");
    return 0;
}

}  // namespace

int dangx_moments_hist_get_dev(dangx_ctx* ctx, int reg, void* counts_dev) {
    if (!ctx || !counts_dev || hist_reg(ctx, reg)) return 1;
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const size_t bytes = sizeof(uint32_t) * (size_t)ctx->dims.npix * dx_hist_words(m->hbins, m->hbits);
    HIPCHK(ctx, hipMemcpyAsync(counts_dev, m->hrec + m->hists[reg].off, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int dangx_moments_hist_get(dangx_ctx* ctx, int reg, void* counts) {
    if (!ctx || !counts || hist_reg(ctx, reg)) return 1;
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const size_t bytes = sizeof(uint32_t) * (size_t)ctx->dims.npix * dx_hist_words(m->hbins, m->hbits);
    HIPCHK(ctx, hipMemcpyAsync(counts, m->hrec + m->hists[reg].off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

static int hist_stat_check(dangx_ctx* ctx, int reg, int stat, int nq, const double* q) {
    if (hist_reg(ctx, reg)) return 1;
    if (stat < 0 || stat > 2) return fail(ctx, "posterior moments: the stat of a histogram must be 0 (quantiles), 1 (mode) or 2 (counted samples)");
    if (stat == 0) {
        if (nq < 1 || nq > DX_HIST_MAX_Q || !q)
            return fail(ctx, "posterior moments: a histogram read-out takes 1 to " + std::to_string(DX_HIST_MAX_Q) + " quantiles");
        for (int j = 0; j < nq; ++j)
            if (!(q[j] > 0.0 && q[j] < 1.0)) return fail(ctx, "posterior moments: every quantile must lie strictly inside (0, 1)");
    }
    return 0;
}

int dangx_moments_hist_stat_dev(dangx_ctx* ctx, int reg, int stat, int nq, const double* q, double* out_dev) {
    if (!ctx || !out_dev || hist_stat_check(ctx, reg, stat, nq, q)) return 1;
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const auto& h = m->hists[reg];
    HistStatArgs a{};
    a.rec = m->hrec + h.off; a.out = out_dev; a.lo = h.lo; a.hi = h.hi; a.n = ctx->dims.npix;
    a.nbins = m->hbins; a.bits = m->hbits; a.stat = stat; a.nq = stat == 0 ? nq : 0;
    for (int j = 0; j < a.nq; ++j) a.q[j] = q[j];
    const unsigned gx = std::max(1u, std::min(nblocks(a.n), 2048u));
    hipLaunchKernelGGL(k_hist_stat, dim3(gx), dim3(BLOCK), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int dangx_moments_hist_stat(dangx_ctx* ctx, int reg, int stat, int nq, const double* q, double* out) {
    if (!ctx || !out || hist_stat_check(ctx, reg, stat, nq, q)) return 1;   // before anything is allocated
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const int rows = stat == 0 ? nq : 1;
    const size_t bytes = sizeof(double) * (size_t)ctx->dims.npix * rows;
    if (bytes > m->hscratch_bytes) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (m->hscratch) (void)hipFree(m->hscratch);
        m->hscratch = nullptr; m->hscratch_bytes = 0;
        HIPCHK(ctx, hipMalloc(&m->hscratch, bytes));
        m->hscratch_bytes = bytes;
    }
    if (dangx_moments_hist_stat_dev(ctx, reg, stat, nq, q, m->hscratch)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(out, m->hscratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_signals(dangx_ctx* ctx, int nsig, const int32_t* spec) {
    if (!ctx || need(ctx)) return 1;
    DxMoments* m = ctx->mom;
    if (m->count != 0)
        return fail(ctx, "posterior moments: dangx_moments_signals is legal only before the first dangx_moments_accumulate after dangx_moments_begin");
    const int ncomp = ctx->dims.ncomp, nmaps = ctx->dims.nmaps;
    int set[MAXC] = {}, global[MAXC] = {};
    for (int l = 0; l < ncomp; ++l) {
        set[l] = ctx->comp_set[l] ? 1 : 0;
        global[l] = is_global_type(ctx->desc[l].type) ? 1 : 0;
    }
    const std::string why = dx_signal_check(nsig, spec, ncomp, ctx->dims.nbands, nmaps, set, global);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_signals: " + why);
    (void)hipSetDevice(ctx->device);
    bool used[MAXC] = {};
    for (int s = 0; s < nsig; ++s) used[spec[3 * s]] = true;
    for (int l = 0; l < ncomp; ++l)   // the chain's maps exist from here on (what dangx_get_amplitude does on first use)
        if (used[l] && ensure_state(ctx, l)) return 1;
    const std::vector<DxSigSeg> plan = dx_signal_plan(nsig, spec, ncomp, ctx->dims.nbands);
    // accumulators: every signal's planes at the 16-byte phase of the first plane of its class, so that the streams line up
    std::vector<DxMoments::Sig> ns;
    long long off = 0;
    for (int s = 0; s < nsig; ++s) {
        DxMoments::Sig sg{spec[3 * s], spec[3 * s + 1], spec[3 * s + 2], 0};
        const double* plane = ctx->amp[sg.comp] + (long long)(sig_k0(dx_signal_class(sg.kind)) - 1) * ctx->dims.npix;
        const long long phase = (long long)((reinterpret_cast<uintptr_t>(plane) >> 3) & 1);
        if ((off & 1) != phase) ++off;
        sg.off = off;
        off += ctx->dims.npix;
        ns.push_back(sg);
    }
    const long long half = off + (off & 1);   // even: the m2 half has the phases of the mean half
    // everything new is allocated before anything old is dropped: a failure leaves the registration as it was
    double* sacc = nullptr;
    SigSeg* d_sig = nullptr;
    auto bail = [&](hipError_t e, const char* what) {
        ctx->err = std::string("posterior moments: dangx_moments_signals: ") + what + ": " + hipGetErrorString(e);
        if (sacc) (void)hipFree(sacc);
        if (d_sig) (void)hipFree(d_sig);
        return 1;
    };
    hipError_t e;
    if (!ns.empty()) {
        if ((e = hipMalloc(&sacc, sizeof(double) * 2 * (size_t)half)) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipMemsetAsync(sacc, 0, sizeof(double) * 2 * (size_t)half, ctx->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
        if ((e = hipMalloc(&d_sig, sizeof(SigSeg) * plan.size())) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    }
    if (m->sacc) (void)hipFree(m->sacc);
    if (m->d_sig) (void)hipFree(m->d_sig);
    m->sacc = sacc; m->d_sig = d_sig; m->sacc_half = half;
    m->sigs = ns;
    m->sig_plan = plan;
    m->sig_table.clear();   // the next accumulation uploads the table
    for (int l = 0; l < MAXC; ++l) {
        m->sig_used[l] = l < ncomp && used[l];
        m->sig_type[l] = m->sig_used[l] ? ctx->desc[l].type : 0;
        m->sig_nind[l] = m->sig_used[l] ? ctx->desc[l].nindices : 0;
    }
    return 0;
}

int dangx_moments_get_signal_dev(dangx_ctx* ctx, int sig, int stat, int ddof, double* out_dev) {
    if (!ctx || !out_dev || signal_get_check(ctx, sig, stat, ddof)) return 1;
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const long long off = m->sigs[sig].off;
    return finish_plane(ctx, m->sacc + off, m->sacc + m->sacc_half + off, stat, (double)(m->count - ddof), out_dev);
}

int dangx_moments_get_signal(dangx_ctx* ctx, int sig, int stat, int ddof, double* out) {
    if (!ctx || !out || signal_get_check(ctx, sig, stat, ddof)) return 1;   // before anything is allocated
    DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const long long np = ctx->dims.npix;
    if (!m->scratch) HIPCHK(ctx, hipMalloc(&m->scratch, sizeof(double) * (size_t)np * ctx->dims.nmaps));
    if (dangx_moments_get_signal_dev(ctx, sig, stat, ddof, m->scratch)) return 1;
    HIPCHK(ctx, hipMemcpyAsync(out, m->scratch, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_end(dangx_ctx* ctx) {
    if (!ctx) return 1;
    (void)hipSetDevice(ctx->device);
    if (ctx->mom) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // no launch may still read the accumulators
    dx_moments_free(ctx);
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// dangx_chains_*: read-outs over the accumulators of SEVERAL chains of one device (definitions in dx_chains_host.h).  Nothing here
// touches an accumulator, a chain or a cache: three read-only kernels combine the per-chain planes and write only the map asked for.
//   k_chains_stat  planes and signals (blockIdx.y = plane, up to three): pooled mean / std, R-hat, W, B/n read K x (mean, m2) --
//                  a stat that does not use one of the two does not load it -- and write one f64: at most (2 K + 1) x 8 B per
//                  element; the pooled ESS reads K x (mean, m2, prev, first, P), (5 K + 1) x 8 B.
//   k_chains_pair  one pair: K x (mean_a, mean_b, C) for the covariance, + K x (m2_a, m2_b) for the correlation.
//   k_chains_hist  a lane sums its pixel's K records piece by piece in 64-bit integers and takes k_hist_stat's steps on the sums.
// The pointers of all chains travel by value (ChainsArgs + DxChainsPar: 1.3 KB of the 4 KB kernel-argument segment).  Pairs of elements are read
// as 16 bytes where every pointer of a plane shares out's 16-byte phase, element by element otherwise (chains whose buffers were
// adopted at different alignments); both forms evaluate the same header functions.  No LDS, no atomics, no scratch.

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

template <int V> struct ChV;
template <> struct ChV<1> {
    static __device__ __forceinline__ void ld(const double* p, double (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void st(double* p, const double (&v)[1]) { *p = v[0]; }
};
template <> struct ChV<2> {
    static __device__ __forceinline__ void ld(const double* p, double (&v)[2]) { const dbl2 t = *(const GD2*)p; v[0] = t.x; v[1] = t.y; }
    static __device__ __forceinline__ void st(double* p, const double (&v)[2]) { *(GD2*)p = dbl2{v[0], v[1]}; }
};

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
    const uintptr_t ao = reinterpret_cast<uintptr_t>(a->out[p]);
    uintptr_t diff = ao & 7;   // out not even at a double's alignment: element by element
    const bool ess = stat == DX_CH_ESS;
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        diff |= (ao ^ reinterpret_cast<uintptr_t>(a->mean[p][k])) | (ao ^ reinterpret_cast<uintptr_t>(a->m2[p][k]));
        if (ess)
            diff |= (ao ^ reinterpret_cast<uintptr_t>(a->prev[p][k])) | (ao ^ reinterpret_cast<uintptr_t>(a->first[p][k])) |
                    (ao ^ reinterpret_cast<uintptr_t>(a->P[p][k]));
    });
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
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const uintptr_t ao = reinterpret_cast<uintptr_t>(a.out);
    uintptr_t diff = ao & 7;
    dx_chains_each<0>(par.K, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        diff |= (ao ^ reinterpret_cast<uintptr_t>(a.ma[k])) | (ao ^ reinterpret_cast<uintptr_t>(a.mb[k])) |
                (ao ^ reinterpret_cast<uintptr_t>(a.qa[k])) | (ao ^ reinterpret_cast<uintptr_t>(a.qb[k])) |
                (ao ^ reinterpret_cast<uintptr_t>(a.C[k]));
    });
    if ((diff & 15) != 0) {   // the two planes (or a chain's adopted buffers) at different 16-byte phases
        for (long long i = gid; i < n; i += stride) chains_pair_item<1>(a, par, stat, i);
        return;
    }
    const long long head = ((ao & 15) != 0 && n > 0) ? 1 : 0;
    const long long npair = (n - head) / 2, tail = head + 2 * npair;
    if (gid == 0 && head) chains_pair_item<1>(a, par, stat, 0);
    if (gid == 1 && tail < n) chains_pair_item<1>(a, par, stat, tail);
    for (long long t = gid; t < npair; t += stride) chains_pair_item<2>(a, par, stat, head + 2 * t);
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
template <class F>
__device__ __forceinline__ void chains_hist_walk(const ChainsHistArgs& a, long long i, int pieces, F f) {
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
    const double width = (a.hi - a.lo) / (double)a.nbins;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * BLOCK) {
        unsigned long long N = 0, best_c = 0;
        int best_b = -1;
        chains_hist_walk(a, i, pieces, [&](unsigned long long c, int b) { N += c; dx_hist_mstep(c, b, best_c, best_b); return false; });
        if (a.stat == 1) { a.out[i] = dx_hist_mode_value(best_b, a.lo, width); continue; }
        if (a.stat == 2) { a.out[i] = (double)N; continue; }
        for (int j = 0; j < a.nq; ++j) {
            double val = (double)NAN;
            if (N > 0) {
                const double target = a.q[j] * (double)N;
                unsigned long long cum = 0;
                chains_hist_walk(a, i, pieces, [&](unsigned long long c, int b) { return dx_hist_qstep(c, b, target, cum, a.lo, width, val); });
            }
            a.out[(long long)j * a.n + i] = val;
        }
    }
}

// ---- host side

struct ChainSet {
    dangx_ctx* const* c;
    int K;
    long long cnt[DX_CHAINS_MAX];
};

int chains_fail(dangx_ctx* const* ctxs, const std::string& msg) { return fail(ctxs[0], "posterior chains: " + msg); }

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

// k_chains_stat on stream 0 between the two joins; a.mean .. a.out of np planes are filled in
int chains_launch(const ChainSet& cs, const ChainsArgs& a, int np, int stat, int ddof) {
    dangx_ctx* c0 = cs.c[0];
    const long long n = c0->dims.npix;
    const DxChainsPar par = dx_chains_par(cs.K, cs.cnt, ddof);
    if (chains_join(cs)) return 1;
    {
        const long long pairs = (n + 1) / 2;
        const unsigned gx = std::max(1u, std::min(nblocks(pairs), (c0->mom->grid_target + np - 1) / np));
        Timed tm(c0, DANGX_K_CHAINS);
        hipLaunchKernelGGL(k_chains_stat, dim3(gx, np), dim3(BLOCK), 0, c0->stream, a, par, n, stat);
        HIPCHK(c0, hipGetLastError());
    }
    return chains_release(cs);
}

int chains_scratch(dangx_ctx* c0) {
    DxMoments* m = c0->mom;
    if (!m->scratch) HIPCHK(c0, hipMalloc(&m->scratch, sizeof(double) * (size_t)c0->dims.npix * c0->dims.nmaps));
    return 0;
}

int chains_get_impl(dangx_ctx* const* ctxs, int nchains, int comp, int what, int stat, int ddof, double* dst, bool to_host, double* out) {
    ChainSet cs{};
    unsigned planes = 0;
    if (chains_open(ctxs, nchains, cs) || chains_planes(cs, comp, what, stat, planes) || chains_counts(cs, stat, ddof, false)) return 1;
    dangx_ctx* c0 = ctxs[0];
    if (what == 0 && is_global_type(c0->desc[comp].type))
        return chains_fail(ctxs, "a template / monopole / hi_fit amplitude is read with dangx_chains_get_template");
    (void)hipSetDevice(c0->device);
    const long long np = c0->dims.npix;
    if (to_host) {
        if (chains_scratch(c0)) return 1;
        dst = c0->mom->scratch;
    }
    ChainsArgs a{};
    int n = 0;
    for (int k = 0; k < c0->dims.nmaps; ++k) {
        if (!((planes >> k) & 1u)) continue;
        for (int j = 0; j < cs.K; ++j) {
            const DxMoments* m = ctxs[j]->mom;
            long long off = -1;
            for (const auto& s : m->segs)
                if (s.comp == comp && s.what == what && s.plane == k) off = s.off;
            if (off < 0) return chains_fail(ctxs, "chain " + std::to_string(j) + ": a plane of this component and what is not selected");
            a.mean[n][j] = m->acc + off;
            a.m2[n][j] = m->acc + m->acc_half + off;
            if (stat == DX_CH_ESS) {
                a.prev[n][j] = m->lag + off;
                a.first[n][j] = m->lag + m->acc_half + off;
                a.P[n][j] = m->lag + 2 * m->acc_half + off;
            }
        }
        a.out[n] = dst + (long long)k * np;
        ++n;
    }
    if (chains_launch(cs, a, n, stat, ddof)) return 1;
    if (to_host) {
        const long long hs = c0->host_stride > 0 ? c0->host_stride : np;
        for (int k = 0; k < c0->dims.nmaps; ++k)
            if ((planes >> k) & 1u)
                HIPCHK(c0, hipMemcpyAsync(out + (long long)k * hs, dst + (long long)k * np, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));
    }
    return 0;
}

int chains_signal_impl(dangx_ctx* const* ctxs, int nchains, int sig, int stat, int ddof, double* dst, bool to_host, double* out) {
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
    if (to_host) {
        if (chains_scratch(c0)) return 1;
        dst = c0->mom->scratch;
    }
    ChainsArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        const DxMoments* m = ctxs[j]->mom;
        a.mean[0][j] = m->sacc + m->sigs[sig].off;
        a.m2[0][j] = m->sacc + m->sacc_half + m->sigs[sig].off;
    }
    a.out[0] = dst;
    if (chains_launch(cs, a, 1, stat, ddof)) return 1;
    if (to_host) {
        HIPCHK(c0, hipMemcpyAsync(out, dst, sizeof(double) * (size_t)c0->dims.npix, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));
    }
    return 0;
}

int chains_pair_impl(dangx_ctx* const* ctxs, int nchains, int pair, int stat, int ddof, double* dst, bool to_host, double* out) {
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    if (stat != 0 && stat != 1) return chains_fail(ctxs, "the stat of a pair must be 0 (covariance) or 1 (correlation)");
    const DxMoments* m0 = ctxs[0]->mom;
    if (pair < 0 || pair >= (int)m0->pairs.size())
        return chains_fail(ctxs, "chain 0: pair index out of range (" + std::to_string(m0->pairs.size()) + " pairs registered)");
    auto same_seg = [](const DxMoments::Seg& x, const DxMoments::Seg& y) { return x.comp == y.comp && x.what == y.what && x.plane == y.plane; };
    for (int k = 1; k < nchains; ++k) {
        const DxMoments* m = ctxs[k]->mom;
        if (pair >= (int)m->pairs.size() || !same_seg(m->segs[m->pairs[pair].a], m0->segs[m0->pairs[pair].a]) ||
            !same_seg(m->segs[m->pairs[pair].b], m0->segs[m0->pairs[pair].b]))
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": pair " + std::to_string(pair) + " is not the registration of chain 0");
    }
    if (chains_counts(cs, stat, ddof, true)) return 1;
    dangx_ctx* c0 = ctxs[0];
    (void)hipSetDevice(c0->device);
    if (to_host) {
        if (chains_scratch(c0)) return 1;
        dst = c0->mom->scratch;
    }
    ChainsPairArgs a{};
    for (int j = 0; j < cs.K; ++j) {
        const DxMoments* m = ctxs[j]->mom;
        const auto& p = m->pairs[pair];
        a.ma[j] = m->acc + m->segs[p.a].off;
        a.mb[j] = m->acc + m->segs[p.b].off;
        a.qa[j] = m->acc + m->acc_half + m->segs[p.a].off;
        a.qb[j] = m->acc + m->acc_half + m->segs[p.b].off;
        a.C[j] = m->pc + p.off;
    }
    a.out = dst;
    const long long n = c0->dims.npix;
    const DxChainsPar par = dx_chains_par(cs.K, cs.cnt, ddof);
    if (chains_join(cs)) return 1;
    {
        const unsigned gx = std::max(1u, std::min(nblocks((n + 1) / 2), c0->mom->grid_target));
        Timed tm(c0, DANGX_K_CHAINS);
        hipLaunchKernelGGL(k_chains_pair, dim3(gx), dim3(BLOCK), 0, c0->stream, a, par, n, stat);
        HIPCHK(c0, hipGetLastError());
    }
    if (chains_release(cs)) return 1;
    if (to_host) {
        HIPCHK(c0, hipMemcpyAsync(out, dst, sizeof(double) * (size_t)c0->dims.npix, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));
    }
    return 0;
}

int chains_hist_impl(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int nq, const double* q, double* dst, bool to_host, double* out) {
    ChainSet cs{};
    if (chains_open(ctxs, nchains, cs)) return 1;
    const DxMoments* m0 = ctxs[0]->mom;
    if (reg < 0 || reg >= (int)m0->hists.size())
        return chains_fail(ctxs, "chain 0: histogram registration out of range (" + std::to_string(m0->hists.size()) + " registered)");
    for (int k = 1; k < nchains; ++k) {
        const DxMoments* m = ctxs[k]->mom;
        bool same = reg < (int)m->hists.size() && m->hbins == m0->hbins && m->hbits == m0->hbits;
        if (same) {
            const auto &h = m->hists[reg], &h0 = m0->hists[reg];
            const auto &s = m->segs[h.seg], &s0 = m0->segs[h0.seg];
            same = s.comp == s0.comp && s.what == s0.what && s.plane == s0.plane && h.lo == h0.lo && h.hi == h0.hi;
        }
        if (!same)
            return chains_fail(ctxs, "chain " + std::to_string(k) + ": histogram registration " + std::to_string(reg) +
                                         " is not the registration of chain 0 (plane, lo, hi, nbins and bits must agree)");
    }
    dangx_ctx* c0 = ctxs[0];
    if (hist_stat_check(c0, reg, stat, nq, q)) return 1;
    (void)hipSetDevice(c0->device);
    const int rows = stat == 0 ? nq : 1;
    const size_t bytes = sizeof(double) * (size_t)c0->dims.npix * rows;
    if (to_host) {
        DxMoments* m = c0->mom;
        if (bytes > m->hscratch_bytes) {
            HIPCHK(c0, hipStreamSynchronize(c0->stream));
            if (m->hscratch) (void)hipFree(m->hscratch);
            m->hscratch = nullptr; m->hscratch_bytes = 0;
            HIPCHK(c0, hipMalloc(&m->hscratch, bytes));
            m->hscratch_bytes = bytes;
        }
        dst = m->hscratch;
    }
    ChainsHistArgs a{};
    for (int j = 0; j < cs.K; ++j) a.rec[j] = ctxs[j]->mom->hrec + ctxs[j]->mom->hists[reg].off;
    a.out = dst; a.lo = m0->hists[reg].lo; a.hi = m0->hists[reg].hi; a.n = c0->dims.npix;
    a.K = cs.K; a.nbins = m0->hbins; a.bits = m0->hbits; a.stat = stat; a.nq = stat == 0 ? nq : 0;
    for (int j = 0; j < a.nq; ++j) a.q[j] = q[j];
    if (chains_join(cs)) return 1;
    {
        const unsigned gx = std::max(1u, std::min(nblocks(a.n), c0->mom->grid_target));
        Timed tm(c0, DANGX_K_CHAINS);
        hipLaunchKernelGGL(k_chains_hist, dim3(gx), dim3(BLOCK), 0, c0->stream, a);
        HIPCHK(c0, hipGetLastError());
    }
    if (chains_release(cs)) return 1;
    if (to_host) {
        HIPCHK(c0, hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));
    }
    return 0;
}

}  // namespace

extern "C" {

int dangx_chains_get_dev(dangx_ctx* const* ctxs, int nchains, int comp, int what, int stat, int ddof, double* out_dev) {
    if (!ctxs || !ctxs[0] || !out_dev) return 1;
    return chains_get_impl(ctxs, nchains, comp, what, stat, ddof, out_dev, false, nullptr);
}

int dangx_chains_get(dangx_ctx* const* ctxs, int nchains, int comp, int what, int stat, int ddof, double* out) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    return chains_get_impl(ctxs, nchains, comp, what, stat, ddof, nullptr, true, out);
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
    if (!ctxs || !ctxs[0] || !out_dev) return 1;
    return chains_signal_impl(ctxs, nchains, sig, stat, ddof, out_dev, false, nullptr);
}

int dangx_chains_get_signal(dangx_ctx* const* ctxs, int nchains, int sig, int stat, int ddof, double* out) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    return chains_signal_impl(ctxs, nchains, sig, stat, ddof, nullptr, true, out);
}

int dangx_chains_get_pair_dev(dangx_ctx* const* ctxs, int nchains, int pair, int stat, int ddof, double* out_dev) {
    if (!ctxs || !ctxs[0] || !out_dev) return 1;
    return chains_pair_impl(ctxs, nchains, pair, stat, ddof, out_dev, false, nullptr);
}

int dangx_chains_get_pair(dangx_ctx* const* ctxs, int nchains, int pair, int stat, int ddof, double* out) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    return chains_pair_impl(ctxs, nchains, pair, stat, ddof, nullptr, true, out);
}

int dangx_chains_hist_stat_dev(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int nq, const double* q, double* out_dev) {
    if (!ctxs || !ctxs[0] || !out_dev) return 1;
    return chains_hist_impl(ctxs, nchains, reg, stat, nq, q, out_dev, false, nullptr);
}

int dangx_chains_hist_stat(dangx_ctx* const* ctxs, int nchains, int reg, int stat, int nq, const double* q, double* out) {
    if (!ctxs || !ctxs[0] || !out) return 1;
    return chains_hist_impl(ctxs, nchains, reg, stat, nq, q, nullptr, true, out);
}

}  // extern "C"
