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
// A registration may instead take its range per pixel from two f64 maps (dangx_moments_hist_range_maps): those registrations go
// into one launch of k_moments_hist_px, which streams lo and hi beside x and forms the bin with the pixel's own bounds, and are
// read by k_hist_stat_px; k_moments_hist and k_hist_stat stay what they were for the registrations with one range per shard.
//
// dangx_moments_signals adds the moments of component signals at a band (definitions in dx_signal_host.h): the sample
// comp_signal(band, pix, plane) = amplitude * sed(indices) of a diffuse component -- what write_maps' output_fg maps hold
// (src/dang_data_mod.f90:596-617) -- and its polarised intensity P = sqrt(Q^2 + U^2), nonlinear in the sampled parameters and so not
// derivable from their moments.  k_moments_signal is a launch of its own behind the others (blockIdx.y = segment: a component
// and plane class with up to 8 bands): a thread reads a pixel's amplitude and index values once, prepares the SED once per plane
// and updates the f64 mean / m2 planes of every registered output of every band of the segment.  Segments with an integrated
// band go to a second launch of the kernel's BP form (the streaming form carries no bandpass code).  Nothing registered: no launch.
//
// dangx_moments_angles adds the posterior polarisation angle of a component's signal at a band (definitions in dx_angle_host.h):
// a circular statistic, so what is accumulated is the running mean of (cos 2psi, sin 2psi) = (sQ, sU) / P of the signals' own
// rounded samples, two f64 planes per angle.  k_moments_angle is a launch of its own behind the signals' (blockIdx.y = segment: a
// component with up to 8 bands; a second launch of the BP form for segments with an integrated band); k_angle_finish reads the
// circular mean, the circular standard deviation and the mean resultant length off the two planes.  Nothing registered: no launch.
//
// dangx_moments_batches adds batched accumulators of registered pixel planes (definitions in dx_batches_host.h): nbatch slots of
// (mean, m2) per plane in an allocation of the library's own.  An accumulation adds ONE launch of k_moments_accum behind the
// others, on the table row of the slot the sample belongs to (inv_n = 1 / its number within the slot); when every slot is full
// k_batches_merge first folds the slots pairwise in place and the batch length doubles.  k_batches_stat reads the slots in one
// pass with running values (discarded burn-in, MCSE, batch-means ESS, split R-hat).  Nothing registered: no launch.
//
// dangx_moments_fit adds the goodness-of-fit maps write_maps leaves beside the components (definitions in dx_fit_host.h): the
// residual at a (band, plane) and the chi^2 map of a plane, quadratic in all sampled parameters at once and so not derivable from
// any other accumulator.  k_moments_fit is ONE launch of its own behind the others (blockIdx.y = plane with an item, at most
// three): a thread builds a pixel's sky column over all bands in LDS, walks the bands once and updates the f64 mean / m2 planes of
// the registered residuals and of the chi^2 map -- no copy of the residual exists in memory.  Nothing registered: no launch.
//
// dangx_moments_section_* read and write one section of all this state in a packed layout (dx_section_host.h: HEAD, the planes of a
// (component, what), a pair, a histogram, a signal, a batch registration, an angle, a fit item) with one hipMemcpyAsync per plane and no kernel, and
// dangx_moments_begin_like makes a context a HOLDER of sections put into it, which the read-outs over several chains accept in
// place of a live chain: what saving / restoring a run and chains in other processes are made of.
//
// The state (DxMoments) and the host helpers are in dx_moments_state.h, the loop over a plane (dx_stream) in dx_stream.h; the
// read-outs over several chains (dangx_chains_*) are a translation unit of their own, dangx_chains.hip.
#include "dx_moments_state.h"
#include "dx_moments_host.h"
#include "dx_hist_host.h"
#define DX_BATCH_UNROLL 4   // k_batches_stat: four slots' loads in flight (79 VGPRs, occupancy 6)
#include "dx_batches_host.h"
#include "dx_section_host.h"
#include "dx_stream.h"

#include <memory>

static_assert(DX_MOM_MAX_PAIRS == DANGX_MAX_PAIRS, "dx_moments_host.h and include/dangx.h disagree");
static_assert(DX_HIST_MAX == DANGX_MAX_HIST && DX_HIST_SIGNAL == DANGX_HIST_SIGNAL, "dx_hist_host.h and include/dangx.h disagree");
static_assert(DX_SIG_MAX == DANGX_MAX_SIGNALS, "dx_signal_host.h and include/dangx.h disagree");
static_assert(DX_ANG_MAX == DANGX_MAX_ANGLES && DX_ANG_MAX_CHAINS == DANGX_MAX_CHAINS, "dx_angle_host.h and include/dangx.h disagree");
static_assert(DX_FIT_MAX == DANGX_MAX_FIT, "dx_fit_host.h and include/dangx.h disagree");
static_assert(DX_SEC_HEAD_BYTES == DANGX_SECTION_HEAD_BYTES, "dx_section_host.h and include/dangx.h disagree");
static_assert(DX_BATCH_MAX == DANGX_MAX_BATCHES && DX_BATCH_MAX_PLANES == DANGX_MAX_BATCH_PLANES, "dx_batches_host.h and include/dangx.h disagree");

namespace {


__device__ __forceinline__ void welford(double x, double& mean, double& m2, double inv_n) {
    const double d = x - mean;
    mean = fma(d, inv_n, mean);
    m2 = fma(d, x - mean, m2);
}

// V consecutive elements of a segment from element i on
template <int V>
__device__ __forceinline__ void accum_item(const MomSeg& s, long long i, double inv_n) {
    double x[V], m[V], q[V];
    ChV<V>::ld(s.x + i, x); ChV<V>::ld(s.mean + i, m); ChV<V>::ld(s.m2 + i, q);
#pragma unroll
    for (int e = 0; e < V; ++e) welford(x[e], m[e], q[e], inv_n);
    ChV<V>::st(s.mean + i, m); ChV<V>::st(s.m2 + i, q);
}

// blockIdx.y = segment; the blocks of a segment stride over its pairs of doubles
__global__ __launch_bounds__(BLOCK) void k_moments_accum(const MomSeg* __restrict__ segs, double inv_n) {
    const MomSeg s = segs[blockIdx.y];
    const bool vec = (((addr(s.x) ^ addr(s.mean)) | (addr(s.mean) ^ addr(s.m2))) & 15) == 0;
    dx_stream(s.n, vec, addr(s.x), [&](long long i) { accum_item<1>(s, i, inv_n); }, [&](long long i) { accum_item<2>(s, i, inv_n); });
}

// Welford's update and the lag-1 state from one read of x.  FIRST (sample 1): r = prev = x, P stays the 0 it was allocated with.
template <bool FIRST>
__device__ __forceinline__ void lag_step(double x, double& mean, double& m2, double& prev, double r, double& P, double inv_n) {
    if (FIRST) prev = x;
    else dx_lag_update(x, prev, r, P);
    welford(x, mean, m2, inv_n);
}

template <bool FIRST, int V>
__device__ __forceinline__ void lag_item(const LagSeg& s, long long i, double inv_n) {
    double x[V], m[V], q[V];
    ChV<V>::ld(s.x + i, x); ChV<V>::ld(s.mean + i, m); ChV<V>::ld(s.m2 + i, q);
    if (FIRST) {   // lag_step<true>: the first and the previous sample are x itself
#pragma unroll
        for (int e = 0; e < V; ++e) welford(x[e], m[e], q[e], inv_n);
        ChV<V>::st(s.prev + i, x); ChV<V>::st(s.first + i, x);
    } else {
        double pv[V], r[V], P[V];
        ChV<V>::ld(s.prev + i, pv); ChV<V>::ld(s.first + i, r); ChV<V>::ld(s.P + i, P);
#pragma unroll
        for (int e = 0; e < V; ++e) lag_step<false>(x[e], m[e], q[e], pv[e], r[e], P[e], inv_n);
        ChV<V>::st(s.prev + i, pv); ChV<V>::st(s.P + i, P);
    }
    ChV<V>::st(s.mean + i, m); ChV<V>::st(s.m2 + i, q);
}

// k_moments_accum with the lag-1 state; the accumulators of a plane share their 16-byte phase by construction (dangx_moments_begin
// / _pairs), so as there only the chain's plane can be off phase
template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_moments_accum_lag(const LagSeg* __restrict__ segs, double inv_n) {
    const LagSeg s = segs[blockIdx.y];
    const uintptr_t am = addr(s.mean);
    const uintptr_t diff = (am ^ addr(s.x)) | (am ^ addr(s.m2)) | (am ^ addr(s.prev)) | (am ^ addr(s.first)) | (am ^ addr(s.P));
    dx_stream(s.n, (diff & 15) == 0, addr(s.x), [&](long long i) { lag_item<FIRST, 1>(s, i, inv_n); },
              [&](long long i) { lag_item<FIRST, 2>(s, i, inv_n); });
}

template <int V>
__device__ __forceinline__ void pair_item(const PairSeg& s, long long i, double inv_n) {
    double a[V], b[V], ma[V], mb[V], c[V];
    ChV<V>::ld(s.xa + i, a); ChV<V>::ld(s.xb + i, b); ChV<V>::ld(s.ma + i, ma); ChV<V>::ld(s.mb + i, mb); ChV<V>::ld(s.C + i, c);
#pragma unroll
    for (int e = 0; e < V; ++e) c[e] = dx_pair_update(a[e], b[e], ma[e], mb[e], c[e], inv_n);
    ChV<V>::st(s.C + i, c);
}

// blockIdx.y = pair.  Reads the means as the PREVIOUS accumulation left them: launched before the kernel that updates them.
// Element by element where the two planes (or an adopted buffer) are at different 16-byte phases.
__global__ __launch_bounds__(BLOCK) void k_moments_pairs(const PairSeg* __restrict__ segs, double inv_n) {
    const PairSeg s = segs[blockIdx.y];
    const uintptr_t ac = addr(s.C);
    const uintptr_t diff = (ac ^ addr(s.xa)) | (ac ^ addr(s.xb)) | (ac ^ addr(s.ma)) | (ac ^ addr(s.mb));
    dx_stream(s.n, (diff & 15) == 0, ac, [&](long long i) { pair_item<1>(s, i, inv_n); }, [&](long long i) { pair_item<2>(s, i, inv_n); });
}

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
    const int words = dx_hist_words(s.nbins, s.bits);
    // element by element only where x is not even at a double's alignment
    dx_stream(s.n, (addr(s.x) & 7) == 0, addr(s.x), [&](long long i) { hist_one(s, words, i, s.x[i]); },
              [&](long long i) {
                  double x[2];
                  ChV<2>::ld(s.x + i, x);
                  hist_one(s, words, i, x[0]);
                  hist_one(s, words, i + 1, x[1]);
              });
}

// hist_one with the pixel's own bounds (dx_hist_pixel_bin: the scale is one IEEE division per sample; an off pixel counts nothing)
__device__ __forceinline__ void hist_one_px(const HistPxSeg& s, int words, long long i, double x, double lo, double hi) {
    const int b = dx_hist_pixel_bin(x, lo, hi, s.nbins);
    if (b < 0) return;
    GU32* w = (GU32*)s.rec + i * words + dx_hist_word_of(b, s.bits);
    *w = *w + dx_hist_one(b, s.bits);
}

// k_moments_hist for the registrations with per-pixel ranges (a launch of its own, only when there are any): lo and hi stream
// beside x, 16 more bytes per pixel, as pairs where the three share their 16-byte phase (the library allocates the maps at the
// phase of the segment's accumulators, which dangx_moments_begin lays out at the phase the chain's plane had then) and element by element otherwise
__global__ __launch_bounds__(BLOCK) void k_moments_hist_px(const HistPxSeg* __restrict__ segs) {
    const HistPxSeg s = segs[blockIdx.y];
    const int words = dx_hist_words(s.nbins, s.bits);
    const uintptr_t ax = addr(s.x);
    const bool vec = (ax & 7) == 0 && (((ax ^ addr(s.lo)) | (ax ^ addr(s.hi))) & 15) == 0;
    dx_stream(s.n, vec, ax, [&](long long i) { hist_one_px(s, words, i, s.x[i], s.lo[i], s.hi[i]); },
              [&](long long i) {
                  double x[2], lo[2], hi[2];
                  ChV<2>::ld(s.x + i, x); ChV<2>::ld(s.lo + i, lo); ChV<2>::ld(s.hi + i, hi);
                  hist_one_px(s, words, i, x[0], lo[0], hi[0]);
                  hist_one_px(s, words, i + 1, x[1], lo[1], hi[1]);
              });
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
// one sample y of an output into pixel i's record of the histogram that reads the output: hist_one's one-word read-modify-write,
// the bin by the pixel's own bounds (dx_hist_pixel_bin; with one range for the shard lo and hi are that range in every pixel, and
// the scale the same one IEEE division the host forms for k_moments_hist: the same integer)
__device__ __forceinline__ void sig_hist_one(uint32_t* rec, int words, int nbins, int bits, long long i, double y, double lo, double hi) {
    const int b = dx_hist_pixel_bin(y, lo, hi, nbins);
    if (b < 0) return;
    GU32* w = (GU32*)rec + i * words + dx_hist_word_of(b, bits);
    *w = *w + dx_hist_one(b, bits);
}

// HIST: after the Welford update of an output the SAME value is binned into the record of the histogram registered on that output
// (SigBand::rec, null = none).  <BP, false> is the kernel as it was and runs whenever no histogram reads a signal; with one, the
// HIST form replaces it in the same launches: no further launch.  The histogram's own uniforms (words, nbins, bits) follow the
// discipline below: parked in VGPRs, and the band's record pointer and range come by vector loads through sv.
template <bool BP, bool HIST>
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
    int hbins = HIST ? s->hbins : 0, hbits = HIST ? s->hbits : 0;
    const SigHistBand* hv = segs[blockIdx.y].hb;
    if (HIST) asm volatile("" : "+v"(hbins), "+v"(hbits), "+v"(hv));
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
                if (HIST) {
                    uint32_t* rec = hv[b].rec[o];
                    if (rec) {
                        const double *lp = hv[b].lo[o], *hp = hv[b].hi[o];
                        const int words = dx_hist_words(hbins, hbits);
                        double l0, l1, h0, h1;
                        if (!lp) { l0 = l1 = hv[b].glo[o]; h0 = h1 = hv[b].ghi[o]; }
                        else if (single) { l0 = l1 = lp[i]; h0 = h1 = hp[i]; }
                        else {
                            const dbl2 lv = *(const GD2*)(lp + i), hv = *(const GD2*)(hp + i);
                            l0 = lv.x; l1 = lv.y; h0 = hv.x; h1 = hv.y;
                        }
                        sig_hist_one(rec, words, hbins, hbits, i, y0, l0, h0);
                        if (!single) sig_hist_one(rec, words, hbins, hbits, i + 1, y1, l1, h1);
                    }
                }
            }
        }
    }
}

typedef const AngSeg __attribute__((address_space(4))) * ang_kptr;   // the segment table through the scalar cache, as sig_kptr

// blockIdx.y = segment: a component with up to DX_ANG_SEG_BANDS bands.  One sample of every registered angle: the running means
// of (c, s) = (sQ, sU) / P (dx_angle_cs), sQ and sU formed exactly as k_moments_signal forms its kinds 1 and 2 -- the same
// sed_prep, sig_sed<BP> and dx_signal_product on the same values.  The item loop is k_moments_signal's with the class fixed to
// Q+U (four evaluation slots e = 2 * (0: Q, 1: U) + (half of the pair)): pairs of pixels where every plane read and both
// accumulators share their 16-byte phase, the odd first / last element alone, element by element otherwise; every slot goes
// through the same code, so a result does not depend on which kind of item held its pixel.  The register discipline is that
// kernel's too: the scalar file belongs to comp_sed's band constants, this kernel's own uniforms are parked in VGPRs.
template <bool BP>
__global__ __launch_bounds__(BLOCK) void k_moments_angle(const Model* __restrict__ Mp, const AngSeg* __restrict__ segs, double inv_n) {
    const Model& M = *Mp;
    const ang_kptr s = reinterpret_cast<ang_kptr>(reinterpret_cast<uintptr_t>(segs + blockIdx.y));
    const Comp& c = M.comp[s->comp];
    const long long n = s->n;
    const long long gid = (long long)blockIdx.x * BLOCK + threadIdx.x, stride = (long long)gridDim.x * BLOCK;
    const int vec = BP ? 0 : s->vec;   // segments with an integrated band: issue bound, element by element
    const long long head = (vec == 2 && n > 0) ? 1 : 0;
    const long long npair = vec ? (n - head) / 2 : 0, tail = head + 2 * npair;   // tail < n: one element after the last pair
    const long long nitems = vec ? npair + head + (tail < n ? 1 : 0) : n;
    int nb = s->nb, nind = s->nind, estep = vec ? 1 : 2;   // estep: the odd slots of an element-by-element item are not evaluated
    long long item_stride = stride, item_end = nitems, pair_end = npair, i_head = head, i_tail = tail;
    const double *pa0 = s->src[0][0], *pt00 = s->src[0][1], *pt01 = s->src[0][2];
    const double *pa1 = s->src[1][0], *pt10 = s->src[1][1], *pt11 = s->src[1][2];
    const AngBand* sv = segs[blockIdx.y].b;
    asm volatile("" : "+v"(item_stride), "+v"(item_end), "+v"(pair_end), "+v"(i_head), "+v"(i_tail), "+v"(inv_n));
    asm volatile("" : "+v"(pa0), "+v"(pt00), "+v"(pt01), "+v"(pa1), "+v"(pt10), "+v"(pt11), "+v"(sv));
    asm volatile("" : "+v"(nb), "+v"(nind), "+v"(estep));
    for (long long t = gid; t < item_end; t += item_stride) {
        const bool single = t >= pair_end;
        const long long i = !single ? i_head + 2 * t : !vec ? t : (t == pair_end && i_head) ? 0 : i_tail;   // the item's first pixel
        double a[4] = {0.0, 0.0, 0.0, 0.0}, t0[4] = {0.0, 0.0, 0.0, 0.0}, t1[4] = {0.0, 0.0, 0.0, 0.0};
        if (single) {
            a[0] = pa0[i]; t0[0] = pt00[i]; t1[0] = pt01[i];
            a[2] = pa1[i]; t0[2] = pt10[i]; t1[2] = pt11[i];
        } else {
            dbl2 v = *(const GD2*)(pa0 + i); a[0] = v.x; a[1] = v.y;
            v = *(const GD2*)(pt00 + i); t0[0] = v.x; t0[1] = v.y;
            v = *(const GD2*)(pt01 + i); t1[0] = v.x; t1[1] = v.y;
            v = *(const GD2*)(pa1 + i); a[2] = v.x; a[3] = v.y;
            v = *(const GD2*)(pt10 + i); t0[2] = v.x; t0[3] = v.y;
            v = *(const GD2*)(pt11 + i); t1[2] = v.x; t1[3] = v.y;
        }
        double q0[4] = {0.0, 0.0, 0.0, 0.0}, q1[4] = {0.0, 0.0, 0.0, 0.0}, q2[4] = {0.0, 0.0, 0.0, 0.0};   // the slots' Prep
#pragma nounroll
        for (int e = 0; e < 4; e += uni(estep)) {
            const Prep pr = sed_prep(c, nind > 0 ? sel4(e, t0[0], t0[1], t0[2], t0[3]) : 0.0, nind > 1 ? sel4(e, t1[0], t1[1], t1[2], t1[3]) : 0.0);
            put4(e, q0, pr.p0); put4(e, q1, pr.p1); put4(e, q2, pr.p2);
        }
        for (int b = 0; b < uni(nb); ++b) {
            const int band = uni(sv[b].band);
            double x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma nounroll
            for (int e = 0; e < 4; e += uni(estep)) {
                const Prep pr = {sel4(e, q0[0], q0[1], q0[2], q0[3]), sel4(e, q1[0], q1[1], q1[2], q1[3]), sel4(e, q2[0], q2[1], q2[2], q2[3])};
                const double sed = sig_sed<BP>(M, c, (int)i + (single ? 0 : (e & 1)), 2 + (e >> 1), band, pr);   // never a pixel past the item
                put4(e, x, dx_signal_product(sel4(e, a[0], a[1], a[2], a[3]), sed));
            }
            double c0, s0, c1, s1;
            dx_angle_cs(x[0], x[2], c0, s0);
            dx_angle_cs(x[1], x[3], c1, s1);   // the second half of a pair; of a single element 0 / 0, never stored
            double* cp = sv[b].C + i;
            double* sp = sv[b].S + i;
            if (single) {
                *cp = dx_angle_mean(c0, *cp, inv_n);
                *sp = dx_angle_mean(s0, *sp, inv_n);
            } else {
                const dbl2 mc = *(GD2*)cp, ms = *(GD2*)sp;
                *(GD2*)cp = dbl2{dx_angle_mean(c0, mc.x, inv_n), dx_angle_mean(c1, mc.y, inv_n)};
                *(GD2*)sp = dbl2{dx_angle_mean(s0, ms.x, inv_n), dx_angle_mean(s1, ms.y, inv_n)};
            }
        }
    }
}

// blockIdx.y = segment: a plane with at least one fit item (at most three).  One sample of every registered residual and of the
// plane's chi^2 map, fused: a thread owns a pixel, builds the plane's sky column over all bands once in LDS ([nb][blockDim.x], as
// k_sky_chisq does -- nb is a run-time number) with load_theta / sed_prep / comp_sed of every component, then walks the bands once:
// the residual and the chi^2 term of the band (dx_fit_host.h's expressions), Welford's update of the band's residual item where
// one is registered, and at the end the update of the chi^2 item at an unmasked pixel.  Every data plane is read once, rms only
// where chi^2 is wanted, and no residual ever lies in memory outside the accumulators.  The accesses are 8 bytes per lane,
// consecutive over the wave (512-byte runs), at any alignment of the caller's buffers: a pixel's result does not depend on the
// shard it is in or on the phase of an adopted buffer.  The accumulator pointers are wave-uniform table entries indexed by the
// band: scalar loads, no register array.  4 waves per SIMD are asked for, as k_sky_chisq asks: left to itself the allocator sits at
// 127 registers, one short of dropping to 3 waves with any small change of the SED helpers.
__global__ __launch_bounds__(BLOCK, 4) void k_moments_fit(const Model* __restrict__ Mp, const FitSeg* __restrict__ segs, double inv_n) {
    extern __shared__ double fit_col[];   // [nb][BS]
    const Model& M = *Mp;
    const FitSeg& s = segs[blockIdx.y];
    const int BS = blockDim.x, tid = threadIdx.x;
    const int npix = M.npix, nb = M.nbands, plane = s.plane, k = plane + 1;
    const bool want_chi = s.chi_mean != nullptr;
    for (long long i0 = (long long)blockIdx.x * BS; i0 < npix; i0 += (long long)gridDim.x * BS) {
        if (i0 + tid >= npix) continue;   // no barrier below: a column belongs to its thread
        const int i = (int)i0 + tid;
        for (int j = 0; j < nb; ++j) fit_col[j * BS + tid] = 0.0;
        for (int l = 0; l < M.ncomp; ++l) {
            const Comp& c = M.comp[l];
            if (c.type == DANGX_MONOPOLE) continue;   // lives in the band offsets (src/dang_data_mod.f90:357-361)
            const double amp = c.amp[(long long)plane * npix + i];
            double t0, t1;
            load_theta(M, c, i, k, t0, t1);
            const Prep pr = sed_prep(c, t0, t1);
            for (int j = 0; j < nb; ++j) {
                const double sed = comp_sed(M, c, i, k, j, pr);
                // comp_signal with the product rounded: the bare sed for T_cmb, template_amplitudes * sed for the global types
                const double x = (c.type == DANGX_TCMB) ? sed : dx_fit_product(is_global_type(c.type) ? c.tamp[plane][j] : amp, sed);
                fit_col[j * BS + tid] = dx_fit_sky_add(fit_col[j * BS + tid], x);
            }
        }
        const bool chi_here = want_chi && !is_masked(M.mask[i]);
        double chi = 0.0;
        for (int j = 0; j < nb; ++j) {
            const long long q = ((long long)j * M.nmaps + plane) * npix + i;
            const double r = dx_fit_residual(plane, M.sig[q], M.offset[j], M.gain[j], fit_col[j * BS + tid]);
            if (chi_here) chi = dx_fit_chi_add(chi, dx_fit_chi_term(r, M.rms[q]));
            double* mp = s.rmean[j];
            if (mp) {
                double* qp = s.rm2[j];
                double m = mp[i], v = qp[i];
                welford(r, m, v, inv_n);
                mp[i] = m; qp[i] = v;
            }
        }
        if (chi_here) {
            double m = s.chi_mean[i], v = s.chi_m2[i];
            welford(dx_fit_chisq(chi, nb), m, v, inv_n);
            s.chi_mean[i] = m; s.chi_m2[i] = v;
        }
    }
}

// one chain's read-out: out = dx_angle_stat(stat, Cbar, Sbar)
__global__ __launch_bounds__(BLOCK) void k_angle_finish(const double* __restrict__ C, const double* __restrict__ S, double* __restrict__ out,
                                                        long long n, int stat) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK)
        out[i] = dx_angle_stat(stat, C[i], S[i]);
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

// a lane walks its own record (dx_hist_readout)
__global__ __launch_bounds__(BLOCK) void k_hist_stat(HistStatArgs a) {
    const GU4* __restrict__ rec = (const GU4*)a.rec;
    const int pieces = dx_hist_words(a.nbins, a.bits) / 4;
    dx_hist_readout<uint32_t>(a, [&](long long i, auto f) { hist_walk(rec, i, pieces, a.bits, f); });
}

struct HistStatPxArgs : HistStatArgs {
    const double* lo_map;   // [n]: the registration's range maps in place of lo, hi
    const double* hi_map;
};

// k_hist_stat of a registration with per-pixel ranges (quantiles and the mode; N needs no range and goes through k_hist_stat)
__global__ __launch_bounds__(BLOCK) void k_hist_stat_px(HistStatPxArgs a) {
    const GU4* __restrict__ rec = (const GU4*)a.rec;
    const int pieces = dx_hist_words(a.nbins, a.bits) / 4;
    dx_hist_readout_impl<true, uint32_t>(a, [&](long long i, auto f) { hist_walk(rec, i, pieces, a.bits, f); });
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

// ---- batched accumulators

// V consecutive elements of every slot of a registration: slots (2t, 2t+1) folded into slot t for t ascending, the upper half zeroed
template <int V>
__device__ __forceinline__ void merge_item(double* base, long long pitch, int nbatch, double halfL, long long i) {
    const int half = nbatch / 2;
    for (int t = 0; t < half; ++t) {
        double mu[V], M[V], m[V], q[V];
        ChV<V>::ld(base + (4LL * t) * pitch + i, mu); ChV<V>::ld(base + (4LL * t + 1) * pitch + i, M);
        ChV<V>::ld(base + (4LL * t + 2) * pitch + i, m); ChV<V>::ld(base + (4LL * t + 3) * pitch + i, q);
#pragma unroll
        for (int e = 0; e < V; ++e) dx_batches_merge(m[e], q[e], halfL, mu[e], M[e]);
        ChV<V>::st(base + (2LL * t) * pitch + i, mu); ChV<V>::st(base + (2LL * t + 1) * pitch + i, M);
    }
    double z[V];
#pragma unroll
    for (int e = 0; e < V; ++e) z[e] = 0.0;
    for (int t = 2 * half; t < 2 * nbatch; ++t) ChV<V>::st(base + (long long)t * pitch + i, z);
}

// blockIdx.y = registration; segs: the table row of slot 0, whose mean is the registration's first plane (planes `pitch` apart:
// mean_0, m2_0, mean_1, ...).  The merge is IN PLACE: one thread owns an element (a pair of elements) in every slot, and walks
// t ascending -- it reads slots 2t and 2t+1 before it writes slot t, and a later step t' > t reads slots 2t', 2t'+1 >= 2t + 2 > t,
// so no step overwrites a source that is still unread (destination t <= 2t).  No second buffer, no atomics, no other thread
// touches the element.
__global__ __launch_bounds__(BLOCK) void k_batches_merge(const MomSeg* __restrict__ segs, long long pitch, int nbatch, double halfL) {
    const MomSeg s = segs[blockIdx.y];
    dx_stream(s.n, true, addr(s.mean), [&](long long i) { merge_item<1>(s.mean, pitch, nbatch, halfL, i); },
              [&](long long i) { merge_item<2>(s.mean, pitch, nbatch, halfL, i); });
}

struct BatchStatArgs {
    const double* base;   // slot 0's mean plane of the registration
    double* out;
    long long pitch, n;
    DxBatchPar par;
};

template <int V>
__device__ __forceinline__ void batch_stat_item(const BatchStatArgs& a, long long i) {
    double r[V];
    dx_batches_stat<V>(a.par, [&](int b, bool want_m2, double (&m)[V], double (&q)[V]) DX_LAMBDA_INLINE {
        ChV<V>::ld(a.base + (2LL * b) * a.pitch + i, m);
        if (want_m2) ChV<V>::ld(a.base + (2LL * b + 1) * a.pitch + i, q);
        else {
#pragma unroll
            for (int e = 0; e < V; ++e) q[e] = 0.0;
        }
    }, r);
    ChV<V>::st(a.out + i, r);
}

// one registration's slots in ONE pass with running values: at most (2 nbatch + 1) x 8 B per element; a stat that does not use
// m2 (mean, MCSE) does not load it.  16-byte accesses where out shares the slots' phase, element by element otherwise.
__global__ __launch_bounds__(BLOCK) void k_batches_stat(BatchStatArgs a) {
    const uintptr_t ao = addr(a.out);
    const bool vec = ((ao & 7) | ((ao ^ addr(a.base)) & 15)) == 0;
    dx_stream(a.n, vec, ao, [&](long long i) { batch_stat_item<1>(a, i); }, [&](long long i) { batch_stat_item<2>(a, i); });
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

// an entry point that reads or writes accumulators of the context's own
int need_live(dangx_ctx* ctx, const char* who) {
    if (need(ctx)) return 1;
    if (ctx->mom->holder)
        return fail(ctx, std::string("posterior moments: ") + who + ": the context is a holder (dangx_moments_begin_like): it has no accumulators of its own, "
                         "only dangx_moments_section_* and dangx_chains_* take it");
    return 0;
}

// The frame of a registration entry point `who` (dangx_moments_pairs / _hist / _signals / _batches).  reg_open: a context with
// accumulators of its own that has accumulated nothing yet, and (tab given) the tables the dx_*_check functions take, from what
// dangx_moments_begin recorded.  reg_close: everything new has been allocated into locals by now; wait for their fills (`wait`:
// something was allocated) and name the entry on failure.  Only after it returns 0 does the caller move the locals in, so a
// failure leaves the registration as it was.
struct RegTables { int nind[MAXC] = {}, global[MAXC] = {}; };

int reg_open(dangx_ctx* ctx, const char* who, RegTables* tab = nullptr) {
    if (!ctx || need_live(ctx, who)) return 1;
    const DxMoments* m = ctx->mom;
    if (m->count != 0)
        return fail(ctx, std::string("posterior moments: ") + who + " is legal only before the first dangx_moments_accumulate after dangx_moments_begin");
    for (int l = 0; tab && l < ctx->dims.ncomp; ++l) {
        tab->nind[l] = m->nind[l];
        tab->global[l] = is_global_type(m->type[l]) ? 1 : 0;
    }
    return 0;
}

int reg_close(dangx_ctx* ctx, const char* who, DevStatus& st, bool wait) {
    if (wait) st.sync(ctx->stream);
    return st.ok() ? 0 : st.fail(ctx, (std::string(who) + ": ").c_str());
}

// the resident plane of a segment as it is now (adopted buffers may have been replaced since begin)
const double* seg_plane(const dangx_ctx* ctx, const DxMoments::Seg& s) {
    const long long np = ctx->dims.npix;
    if (s.what == 0) return ctx->amp[s.comp] + (long long)s.plane * np;
    return ctx->idx[s.comp] + ((long long)(s.what - 1) * ctx->dims.nmaps + s.plane) * np;
}

// checks of a get: planes of (comp, what) that are selected -> bit k = plane k+1
int get_planes(dangx_ctx* ctx, int comp, int what, int stat, int ddof, unsigned& planes) {
    if (need_live(ctx, "dangx_moments_get")) return 1;
    DxMoments* m = ctx->mom;
    if (comp < 0 || comp >= ctx->dims.ncomp) return fail(ctx, "posterior moments: component index out of range");
    if (what < 0 || what > DANGX_MAX_IND) return fail(ctx, "posterior moments: what must be 0 (amplitude) or 1 + index number");
    if (stat < 0 || stat > 3)
        return fail(ctx, "posterior moments: stat must be 0 (mean), 1 (standard deviation), 2 (lag-1 autocorrelation) or 3 (effective sample size)");
    if (stat >= 2 && !m->lag1)
        return fail(ctx, "posterior moments: the lag-1 autocorrelation is not tracked (dangx_moments_pairs with lag1 != 0 was not called)");
    if (count_check(ctx, stat == 1 ? "standard deviation" : nullptr, ddof)) return 1;
    planes = (unsigned)(m->sel[comp] >> (what == 0 ? 0 : 3 + 3 * (what - 1))) & 7u;
    if (!planes) return fail(ctx, "posterior moments: nothing selected for this component and what");
    return 0;
}

// k_moments_finish of the selected planes of (comp, what) into dst ([nmaps][npix], device)
int finish(dangx_ctx* ctx, int comp, int what, int stat, int ddof, unsigned planes, double* dst) {
    const DxMoments* m = ctx->mom;
    const long long n = ctx->dims.npix;
    FinishLagArgs l{};   // stat >= 2: rho1 / ESS from the lag-1 state
    FinishArgs a{};
    int np = 0;
    for (const auto& s : m->segs) {
        if (s.comp != comp || s.what != what || !((planes >> s.plane) & 1u)) continue;
        a.mean[np] = l.mean[np] = m->mean(s);
        a.m2[np] = l.m2[np] = m->m2(s);
        a.out[np] = l.out[np] = dst + (long long)s.plane * n;
        if (stat >= 2) { l.prev[np] = m->prev(s); l.first[np] = m->first(s); l.P[np] = m->P(s); }
        ++np;
    }
    const dim3 grid(std::max(1u, std::min(nblocks(n), 1024u)), np);
    if (stat >= 2) {
        l.n = n; l.stat = stat; l.cnt = (double)m->count;
        hipLaunchKernelGGL(k_moments_finish_lag, grid, dim3(BLOCK), 0, ctx->stream, l);
    } else {
        a.n = n; a.stat = stat; a.dn = (double)(m->count - ddof);
        hipLaunchKernelGGL(k_moments_finish, grid, dim3(BLOCK), 0, ctx->stream, a);
    }
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
        s.hbins = m->hbins; s.hbits = m->hbits;
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
                sb.mean[o] = m->mean(m->sigs[sg]);
                sb.m2[o] = m->m2(m->sigs[sg]);
                see(sb.mean[o]); see(sb.m2[o]);
                for (const auto& h : m->hists) {   // the histogram that reads this signal, if any
                    if (h.sig != sg) continue;
                    SigHistBand& sh = s.hb[b];
                    sh.rec[o] = m->records(h);
                    if (h.kind == DX_HIST_RANGE_PIXEL) {
                        sh.lo[o] = m->range_lo(h); sh.hi[o] = m->range_hi(h);
                        see(sh.lo[o]); see(sh.hi[o]);
                    } else {
                        sh.glo[o] = h.lo; sh.ghi[o] = h.hi;
                    }
                }
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

// the device table of the registered angles for the chain's planes as they are now: delta-band segments first
// (k_moments_angle<false>), then those with an integrated band; returns the number of the first kind
size_t ang_table(const dangx_ctx* ctx, const DxMoments* m, std::vector<AngSeg>& t) {
    const long long np = ctx->dims.npix;
    const int nmaps = ctx->dims.nmaps;
    t.clear();
    size_t ndelta = 0;
    for (int pass = 0; pass < 2; ++pass)
    for (const DxAngSeg& ps : m->ang_plan) {
        bool bp = false;
        for (int b = 0; b < ps.nb; ++b) bp = bp || ctx->hm.band[ps.band[b]].n != 0;
        if (bp != (pass == 1)) continue;
        if (!bp) ++ndelta;
        AngSeg s;
        std::memset(&s, 0, sizeof s);   // the tables are compared as bytes
        s.amp = ctx->amp[ps.comp];
        s.idx = ctx->idx[ps.comp];
        s.n = np;
        s.comp = ps.comp; s.nb = ps.nb;
        s.nind = ctx->desc[ps.comp].nindices;
        uintptr_t phase = 0, diff = 0;   // diff: bit 3 set when two addresses differ in their 16-byte phase
        bool first = true;
        auto see = [&](const double* q) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(q);
            if (first) { phase = a; first = false; }
            diff |= (a ^ phase) & 15;
        };
        for (int b = 0; b < ps.nb; ++b) {
            const auto& ag = m->angs[ps.ang[b]];
            s.b[b].band = ps.band[b];
            s.b[b].C = m->angC(ag);
            s.b[b].S = m->angS(ag);
            see(s.b[b].C); see(s.b[b].S);
        }
        for (int k = 0; k < 2; ++k) {
            const long long plane = 1 + k;   // Q, U
            for (int q = 0; q < 3; ++q) {
                const bool has = q == 0 || q - 1 < s.nind;
                s.src[k][q] = !has ? s.amp + plane * np : q == 0 ? s.amp + plane * np : s.idx + ((long long)(q - 1) * nmaps + plane) * np;
                see(s.src[k][q]);
            }
        }
        s.vec = diff ? 0 : ((phase & 15) ? 2 : 1);
        t.push_back(s);
    }
    return ndelta;
}

// the device table of the registered fit items: one segment per plane with items
void fit_table(const DxMoments* m, std::vector<FitSeg>& t) {
    t.clear();
    for (const DxFitSeg& ps : m->fit_plan) {
        FitSeg s;
        std::memset(&s, 0, sizeof s);   // the tables are compared as bytes
        s.plane = ps.plane;
        if (ps.chi >= 0) { s.chi_mean = m->mean(m->fits[ps.chi]); s.chi_m2 = m->m2(m->fits[ps.chi]); }
        for (size_t j = 0; j < ps.res.size() && j < (size_t)MAXB; ++j)
            if (ps.res[j] >= 0) { s.rmean[j] = m->mean(m->fits[ps.res[j]]); s.rm2[j] = m->m2(m->fits[ps.res[j]]); }
        t.push_back(s);
    }
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
    if (need_live(ctx, "dangx_moments_get_signal")) return 1;
    const DxMoments* m = ctx->mom;
    if (sig < 0 || sig >= (int)m->sigs.size())
        return fail(ctx, "posterior moments: signal index out of range (" + std::to_string(m->sigs.size()) + " signals registered)");
    if (stat != 0 && stat != 1) return fail(ctx, "posterior moments: the stat of a signal must be 0 (mean) or 1 (standard deviation)");
    return count_check(ctx, stat == 1 ? "standard deviation" : nullptr, ddof);
}

int hist_reg(dangx_ctx* ctx, int reg) {
    if (need(ctx)) return 1;
    const DxMoments* m = ctx->mom;
    if (reg < 0 || reg >= (int)m->hists.size())
        return fail(ctx, "posterior moments: histogram registration out of range (" + std::to_string(m->hists.size()) + " registered)");
    return count_check(ctx, nullptr, 0);
}

}  // namespace

int dx_hist_stat_check(dangx_ctx* ctx, int reg, int stat, int nq, const double* q) {
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

void dx_moments_free(dangx_ctx* ctx) {
    delete ctx->mom;   // its device buffers go with it
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
    std::unique_ptr<DxMoments> m(new DxMoments());   // becomes the context's only when everything below succeeded
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
                s.id = (int)m->segs.size();
                off += ctx->dims.npix;
                m->segs.push_back(s);
            }
    }
    m->acc_half = off + (off & 1);   // even: the m2 half has the phases of the mean half
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || ncu <= 0) ncu = 256;
    m->grid_target = 8u * (unsigned)ncu;
    DevStatus st;
    if (!m->segs.empty()) {
        m->acc.zeros(2 * (size_t)m->acc_half, ctx->stream, st);
        m->d_table.alloc(m->segs.size(), st);
        st.sync(ctx->stream);
    }
    if (!st.ok()) return st.fail(ctx, "");   // what a previous begin left stays
    dx_moments_free(ctx);   // calling begin again starts over
    ctx->mom = m.release();
    return 0;
}

int dangx_moments_pairs(dangx_ctx* ctx, int lag1, int npairs, const int32_t* pairs) {
    RegTables tab;
    if (reg_open(ctx, "dangx_moments_pairs", &tab)) return 1;
    DxMoments* m = ctx->mom;
    const std::string why = dx_pairs_check(npairs, pairs, ctx->dims.ncomp, ctx->dims.nmaps, m->sel, tab.nind, tab.global);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_pairs: " + why);
    std::vector<DxMoments::Pair> np;
    long long off = 0;
    for (int p = 0; p < npairs; ++p) {
        const int32_t* q = pairs + 6 * p;
        DxMoments::Pair pr{m->find_seg(q[0], q[1], q[2]), m->find_seg(q[3], q[4], q[5]), 0};
        if (pr.a < 0 || pr.b < 0) return fail(ctx, "posterior moments: dangx_moments_pairs: pair " + std::to_string(p) + ": a plane that is not selected");
        if ((off & 1) != (m->segs[pr.a].off & 1)) ++off;
        pr.off = off;
        pr.id = p;
        off += ctx->dims.npix;
        np.push_back(pr);
    }
    (void)hipSetDevice(ctx->device);
    // everything new is allocated before anything old is dropped (reg_close): the new buffers are locals that free themselves
    DevBuf<double> lag, pc;
    DevBuf<LagSeg> d_lag;
    DevBuf<PairSeg> d_pairs;
    DevStatus st;
    if (lag1 && !m->segs.empty()) {
        lag.zeros(3 * (size_t)m->acc_half, ctx->stream, st);
        d_lag.alloc(m->segs.size(), st);
    }
    if (!np.empty()) {
        pc.zeros((size_t)off, ctx->stream, st);
        d_pairs.alloc(np.size(), st);
    }
    if (reg_close(ctx, "dangx_moments_pairs", st, true)) return 1;
    m->lag = std::move(lag); m->d_lag = std::move(d_lag); m->pc = std::move(pc); m->d_pairs = std::move(d_pairs);
    m->lag1 = lag1 != 0;
    m->pairs = np;
    m->table.clear();   // the next accumulation uploads the tables
    std::memset(m->tm_prev, 0, sizeof m->tm_prev);
    std::memset(m->tm_first, 0, sizeof m->tm_first);
    std::memset(m->tm_P, 0, sizeof m->tm_P);
    return 0;
}

int dangx_moments_accumulate(dangx_ctx* ctx) {
    if (!ctx || need_live(ctx, "dangx_moments_accumulate")) return 1;
    DxMoments* m = ctx->mom;
    for (int l = 0; l < ctx->dims.ncomp; ++l)
        if (m->sel[l] && (!ctx->comp_set[l] || ctx->desc[l].type != m->type[l] || ctx->desc[l].nindices != m->nind[l]))
            return fail(ctx, "posterior moments: component " + std::to_string(l) + " changed type or nindices since dangx_moments_begin");
    for (int l = 0; l < ctx->dims.ncomp; ++l)
        if (m->sig_used[l] && (!ctx->comp_set[l] || ctx->desc[l].type != m->sig_type[l] || ctx->desc[l].nindices != m->sig_nind[l]))
            return fail(ctx, "posterior moments: component " + std::to_string(l) + " changed type or nindices since dangx_moments_signals");
    for (int l = 0; l < ctx->dims.ncomp; ++l)
        if (m->ang_used[l] && (!ctx->comp_set[l] || ctx->desc[l].type != m->ang_type[l] || ctx->desc[l].nindices != m->ang_nind[l]))
            return fail(ctx, "posterior moments: component " + std::to_string(l) + " changed type or nindices since dangx_moments_angles");
    if (!m->hists.empty()) {   // no counter ever wraps: refused before anything is touched
        const std::string why = dx_hist_limit_check(m->count + 1, m->hbits);
        if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_accumulate: " + why);
        for (const auto& h : m->hists)
            if (h.kind == DX_HIST_RANGE_PIXEL && !h.have_maps)
                return fail(ctx, "posterior moments: dangx_moments_accumulate: histogram registration " + std::to_string(h.id) +
                                     " declared per-pixel ranges and has no maps (dangx_moments_hist_range_maps was not called for it)");
    }
    (void)hipSetDevice(ctx->device);
    if ((!m->sigs.empty() || !m->angs.empty() || !m->fits.empty()) && sync_model(ctx)) return 1;   // the SEDs read the device model: current before anything is launched
    const double inv_n = 1.0 / (double)(m->count + 1);
    const long long pairs = (ctx->dims.npix + 1) / 2;   // the items of a launch that strides over pairs of pixels
    if (!m->segs.empty()) {
        std::vector<MomSeg> t(m->segs.size());
        for (size_t i = 0; i < t.size(); ++i) {
            const auto& s = m->segs[i];
            t[i] = MomSeg{seg_plane(ctx, s), m->mean(s), m->m2(s), (long long)ctx->dims.npix};
        }
        bool same = t.size() == m->table.size();
        for (size_t i = 0; same && i < t.size(); ++i) same = t[i].x == m->table[i].x;
        if (!same) {   // first accumulation, or a component's buffers were adopted again: one upload (and a host wait) here only
            HIPCHK(ctx, hipMemcpyAsync(m->d_table, t.data(), sizeof(MomSeg) * t.size(), hipMemcpyHostToDevice, ctx->stream));
            std::vector<LagSeg> tl;
            std::vector<PairSeg> tp;
            if (m->d_lag) {
                for (size_t i = 0; i < t.size(); ++i) {
                    const auto& s = m->segs[i];
                    tl.push_back(LagSeg{t[i].x, t[i].mean, t[i].m2, m->prev(s), m->first(s), m->P(s), t[i].n});
                }
                HIPCHK(ctx, hipMemcpyAsync(m->d_lag, tl.data(), sizeof(LagSeg) * tl.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            if (m->d_pairs) {
                for (const auto& p : m->pairs)
                    tp.push_back(PairSeg{t[p.a].x, t[p.b].x, t[p.a].mean, t[p.b].mean, m->C(p), (long long)ctx->dims.npix});
                HIPCHK(ctx, hipMemcpyAsync(m->d_pairs, tp.data(), sizeof(PairSeg) * tp.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            std::vector<HistSeg> th;
            std::vector<HistPxSeg> thp;
            if (m->d_hist) {
                for (const auto& h : m->hists) {
                    if (h.sig >= 0) continue;   // a signal's histogram is filled by k_moments_signal (sig_table)
                    if (h.kind == DX_HIST_RANGE_PIXEL)
                        thp.push_back(HistPxSeg{t[h.seg].x, m->records(h), m->range_lo(h), m->range_hi(h), (long long)ctx->dims.npix, m->hbins, m->hbits});
                    else
                        th.push_back(HistSeg{t[h.seg].x, m->records(h), h.lo, h.hi, dx_hist_scale(h.lo, h.hi, m->hbins), (long long)ctx->dims.npix,
                                             m->hbins, m->hbits});
                }
                if (!th.empty())
                    HIPCHK(ctx, hipMemcpyAsync(m->d_hist, th.data(), sizeof(HistSeg) * th.size(), hipMemcpyHostToDevice, ctx->stream));
                if (!thp.empty())
                    HIPCHK(ctx, hipMemcpyAsync(m->d_histpx, thp.data(), sizeof(HistPxSeg) * thp.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            std::vector<MomSeg> tb;
            if (m->d_batch) {   // every slot's row at once: moving on to the next slot needs no upload
                for (int b = 0; b < m->nbatch; ++b)
                    for (const auto& r : m->batches) tb.push_back(MomSeg{t[r.seg].x, m->bmean(r, b), m->bm2(r, b), (long long)ctx->dims.npix});
                HIPCHK(ctx, hipMemcpyAsync(m->d_batch, tb.data(), sizeof(MomSeg) * tb.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            m->table = t;
        }
        if (!m->pairs.empty()) {   // the cross terms read the means of the previous accumulation: a launch of its own, first
            const unsigned npr = (unsigned)m->pairs.size();
            Timed tm(ctx, DANGX_K_MOMENTS, 2);   // the profile tells them apart by their plane count: two planes per element
            hipLaunchKernelGGL(k_moments_pairs, dim3(m->grid_for(pairs, npr), npr), dim3(BLOCK), 0, ctx->stream, (const PairSeg*)m->d_pairs, inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
        const unsigned nseg = (unsigned)t.size(), gx = m->grid_for(pairs, nseg);
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
        const unsigned npx = (unsigned)m->nhist_px, nreg = (unsigned)m->hists.size() - npx - (unsigned)m->nhist_sig;   // state planes only
        if (nreg) {
            Timed tm(ctx, DANGX_K_HIST);
            hipLaunchKernelGGL(k_moments_hist, dim3(m->grid_for(pairs, nreg), nreg), dim3(BLOCK), 0, ctx->stream, (const HistSeg*)m->d_hist);
            HIPCHK(ctx, hipGetLastError());
        }
        if (npx) {   // the registrations with per-pixel ranges: the form that streams lo and hi beside x
            Timed tm(ctx, DANGX_K_HIST, 2);   // the profile tells the two forms apart by this mark
            hipLaunchKernelGGL(k_moments_hist_px, dim3(m->grid_for(pairs, npx), npx), dim3(BLOCK), 0, ctx->stream, (const HistPxSeg*)m->d_histpx);
            HIPCHK(ctx, hipGetLastError());
        }
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
        if (ndelta) {
            const unsigned nseg = (unsigned)ndelta;
            Timed tm(ctx, DANGX_K_SIGNAL);
            // a histogram reads a signal: the HIST form in place of the plain one, in the same launch
            auto kern = m->nhist_sig ? k_moments_signal<false, true> : k_moments_signal<false, false>;
            hipLaunchKernelGGL(kern, dim3(m->grid_for(pairs, nseg), nseg), dim3(BLOCK), 0, ctx->stream, (const Model*)ctx->dm,
                               (const SigSeg*)m->d_sig, inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
        if (t.size() > ndelta) {   // segments with an integrated band: element by element
            const unsigned nseg = (unsigned)(t.size() - ndelta);
            Timed tm(ctx, DANGX_K_SIGNAL, 2);   // the profile tells the two forms apart by this mark
            auto kern = m->nhist_sig ? k_moments_signal<true, true> : k_moments_signal<true, false>;
            hipLaunchKernelGGL(kern, dim3(m->grid_for(ctx->dims.npix, nseg), nseg), dim3(BLOCK), 0, ctx->stream, (const Model*)ctx->dm,
                               (const SigSeg*)(m->d_sig + ndelta), inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    if (!m->angs.empty()) {   // the polarisation angles: a launch of their own behind the signals', independent of everything above
        std::vector<AngSeg> t;
        const size_t ndelta = ang_table(ctx, m, t);
        const bool same = t.size() == m->ang_table.size() && std::memcmp(t.data(), m->ang_table.data(), sizeof(AngSeg) * t.size()) == 0;
        if (!same) {   // first accumulation, a component's buffers adopted again or a band's bandpass replaced: one upload (and a host wait)
            HIPCHK(ctx, hipMemcpyAsync(m->d_ang, t.data(), sizeof(AngSeg) * t.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            m->ang_table = t;
        }
        if (ndelta) {
            const unsigned nseg = (unsigned)ndelta;
            Timed tm(ctx, DANGX_K_ANGLE);
            hipLaunchKernelGGL(k_moments_angle<false>, dim3(m->grid_for(pairs, nseg), nseg), dim3(BLOCK), 0, ctx->stream, (const Model*)ctx->dm,
                               (const AngSeg*)m->d_ang, inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
        if (t.size() > ndelta) {   // segments with an integrated band: element by element
            const unsigned nseg = (unsigned)(t.size() - ndelta);
            Timed tm(ctx, DANGX_K_ANGLE, 2);   // the profile tells the two forms apart by this mark
            hipLaunchKernelGGL(k_moments_angle<true>, dim3(m->grid_for(ctx->dims.npix, nseg), nseg), dim3(BLOCK), 0, ctx->stream,
                               (const Model*)ctx->dm, (const AngSeg*)(m->d_ang + ndelta), inv_n);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    if (!m->fits.empty()) {   // the residuals and chi^2 maps: one launch of their own, independent of everything above
        std::vector<FitSeg> t;
        fit_table(m, t);
        const bool same = t.size() == m->fit_table.size() && std::memcmp(t.data(), m->fit_table.data(), sizeof(FitSeg) * t.size()) == 0;
        if (!same) {   // first accumulation: one upload (and a host wait); the chain's planes come through the device model
            HIPCHK(ctx, hipMemcpyAsync(m->d_fit, t.data(), sizeof(FitSeg) * t.size(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            m->fit_table = t;
        }
        int bs = BLOCK;   // the sky column [nbands][bs] within 32 KiB of LDS, as the launch of k_sky_chisq sizes it
        while (bs > 64 && (size_t)ctx->hm.nbands * bs * sizeof(double) > 32 * 1024) bs >>= 1;
        const unsigned nseg = (unsigned)t.size();
        const unsigned gx = std::max(1u, std::min(nblocks(ctx->dims.npix, bs), (m->grid_target * (unsigned)(BLOCK / bs) + nseg - 1) / nseg));
        Timed tm(ctx, DANGX_K_FIT);
        hipLaunchKernelGGL(k_moments_fit, dim3(gx, nseg), dim3(bs), (size_t)ctx->hm.nbands * bs * sizeof(double), ctx->stream,
                           (const Model*)ctx->dm, (const FitSeg*)m->d_fit, inv_n);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!m->batches.empty()) {   // the batched accumulators: k_moments_accum on the row of the slot this sample belongs to
        const unsigned nreg = (unsigned)m->batches.size(), gx = m->grid_for(pairs, nreg);
        if (m->count / m->batch_len == m->nbatch) {   // every slot is full: merged pairwise in place, and the batch length doubles
            Timed tm(ctx, DANGX_K_BATCH, 2);   // the profile tells a merge from an accumulation by this mark
            hipLaunchKernelGGL(k_batches_merge, dim3(gx, nreg), dim3(BLOCK), 0, ctx->stream, (const MomSeg*)m->d_batch, m->bpitch, m->nbatch,
                               0.5 * (double)m->batch_len);
            HIPCHK(ctx, hipGetLastError());
            m->batch_len *= 2;
        }
        const long long b = m->count / m->batch_len, j = m->count % m->batch_len + 1;
        Timed tm(ctx, DANGX_K_BATCH);
        hipLaunchKernelGGL(k_moments_accum, dim3(gx, nreg), dim3(BLOCK), 0, ctx->stream, (const MomSeg*)(m->d_batch + b * nreg), 1.0 / (double)j);
        HIPCHK(ctx, hipGetLastError());
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

// Every read-out below is one implementation; `out` is a device buffer, or with to_host a host array (ReadOut).  The checks come
// before anything is allocated.
static int get_impl(dangx_ctx* ctx, int comp, int what, int stat, int ddof, double* out, bool to_host) {
    if (!ctx || !out) return 1;
    unsigned planes = 0;
    if (get_planes(ctx, comp, what, stat, ddof, planes)) return 1;
    if (what == 0 && is_global_type(ctx->desc[comp].type))
        return fail(ctx, "posterior moments: a template / monopole / hi_fit amplitude is read with dangx_moments_get_template");
    (void)hipSetDevice(ctx->device);
    const long long np = ctx->dims.npix;
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)np * ctx->dims.nmaps) || finish(ctx, comp, what, stat, ddof, planes, ro.dst)) return 1;
    return ro.close(planes, ctx->dims.nmaps, np, ctx->host_stride > 0 ? ctx->host_stride : np);
}

int dangx_moments_get_dev(dangx_ctx* ctx, int comp, int what, int stat, int ddof, double* out_dev) {
    return get_impl(ctx, comp, what, stat, ddof, out_dev, false);
}

int dangx_moments_get(dangx_ctx* ctx, int comp, int what, int stat, int ddof, double* out) {
    return get_impl(ctx, comp, what, stat, ddof, out, true);
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

static int get_pair_impl(dangx_ctx* ctx, int pair, int stat, int ddof, double* out, bool to_host) {
    if (!ctx || !out || need_live(ctx, "dangx_moments_get_pair")) return 1;
    const DxMoments* m = ctx->mom;
    if (pair < 0 || pair >= (int)m->pairs.size())
        return fail(ctx, "posterior moments: pair index out of range (" + std::to_string(m->pairs.size()) + " pairs registered)");
    if (stat != 0 && stat != 1) return fail(ctx, "posterior moments: the stat of a pair must be 0 (covariance) or 1 (correlation)");
    if (count_check(ctx, stat == 0 ? "covariance" : nullptr, ddof)) return 1;
    (void)hipSetDevice(ctx->device);
    const auto& p = m->pairs[pair];
    const long long n = ctx->dims.npix;
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    const unsigned gx = std::max(1u, std::min(nblocks(n), 1024u));
    hipLaunchKernelGGL(k_moments_finish_pair, dim3(gx), dim3(BLOCK), 0, ctx->stream, (const double*)m->C(p),
                       (const double*)m->m2(m->segs[p.a]), (const double*)m->m2(m->segs[p.b]), ro.dst, n, stat, (double)(m->count - ddof));
    HIPCHK(ctx, hipGetLastError());
    return ro.close(n);
}

int dangx_moments_get_pair_dev(dangx_ctx* ctx, int pair, int stat, int ddof, double* out_dev) {
    return get_pair_impl(ctx, pair, stat, ddof, out_dev, false);
}

int dangx_moments_get_pair(dangx_ctx* ctx, int pair, int stat, int ddof, double* out) {
    return get_pair_impl(ctx, pair, stat, ddof, out, true);
}

int dangx_moments_hist(dangx_ctx* ctx, int nreg, const int32_t* planes, const double* range, int nbins, int bits) {
    RegTables tab;
    if (reg_open(ctx, "dangx_moments_hist", &tab)) return 1;
    DxMoments* m = ctx->mom;
    const int ncomp = ctx->dims.ncomp;
    const int* nind = tab.nind;
    // the ranges with the defaults filled in: an index plane's is that index's uni_prior as the descriptor holds it now
    const int nr = std::max(0, std::min(nreg, DX_HIST_MAX));
    std::vector<double> rg(2 * (size_t)nr, 0.0);
    std::vector<int> has(nr, 0), kind(nr, DX_HIST_RANGE_GLOBAL);
    for (int r = 0; planes && r < nr; ++r) {
        const int l = planes[3 * r], w = planes[3 * r + 1];
        if (range && !std::isnan(range[2 * r])) {
            rg[2 * r] = range[2 * r]; rg[2 * r + 1] = range[2 * r + 1];
            has[r] = 1;
            kind[r] = dx_hist_range_kind(rg[2 * r], rg[2 * r + 1]);   // {-inf, +inf}: per-pixel maps follow (dangx_moments_hist_range_maps)
        } else if (w == DX_HIST_SIGNAL) {
            // a signal has no default range: dx_hist_check names it
        } else if (l >= 0 && l < ncomp && w >= 1 && w <= nind[l] && w <= DANGX_MAX_IND) {
            rg[2 * r] = ctx->desc[l].uni_prior[w - 1][0]; rg[2 * r + 1] = ctx->desc[l].uni_prior[w - 1][1];
            has[r] = 1;
        } else if (w != 0) {
            has[r] = 1;   // out of range: dx_hist_check names it
        }
    }
    const std::string why = dx_hist_check(nreg, planes, rg.data(), has.data(), nbins, bits, ncomp, ctx->dims.nmaps, m->sel, nind, tab.global, kind.data(),
                                          (int)m->sigs.size());
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_hist: " + why);
    const long long np = ctx->dims.npix, words = dx_hist_words(nbins, bits);
    const long long pitch = np + (np & 1);   // even: hi at the phase of lo
    std::vector<DxMoments::Hist> nh;
    long long off = 0;   // in 32-bit words; every registration's block starts at a multiple of 256 bytes
    long long roff = 0;  // in doubles: the range maps of the per-pixel registrations, each pair at the phase of its segment's accumulators (Seg::off & 1), which dangx_moments_begin gave the phase of the chain's plane: the invariant k_moments_accum relies on too
    int npx = 0, nhs = 0, nmaps_regs = 0;
    for (int r = 0; r < nreg; ++r) {
        const bool signal = planes[3 * r + 1] == DX_HIST_SIGNAL;
        const int seg = signal ? -1 : m->find_seg(planes[3 * r], planes[3 * r + 1], planes[3 * r + 2]);
        if (!signal && seg < 0) return fail(ctx, "posterior moments: dangx_moments_hist: registration " + std::to_string(r) + ": a plane that is not selected");
        DxMoments::Hist h{seg, rg[2 * r], rg[2 * r + 1], off, r};
        h.kind = kind[r];
        if (signal) { h.sig = planes[3 * r]; ++nhs; }
        if (h.kind == DX_HIST_RANGE_PIXEL) {   // at the phase of what the kernel streams beside the maps: the accumulators of the plane or of the signal
            if ((roff & 1) != ((signal ? m->sigs[h.sig].off : m->segs[seg].off) & 1)) ++roff;
            h.roff = roff;
            roff += 2 * pitch;
            ++nmaps_regs;
            if (!signal) ++npx;
        }
        nh.push_back(h);
        off += (np * words + 63) / 64 * 64;
    }
    (void)hipSetDevice(ctx->device);
    // everything new is allocated before anything old is dropped (reg_close)
    DevBuf<uint32_t> hrec;
    DevBuf<HistSeg> d_hist;
    DevBuf<double> hrange;
    DevBuf<HistPxSeg> d_histpx;
    DevStatus st;
    if (!nh.empty()) {
        hrec.zeros((size_t)off, ctx->stream, st);
        d_hist.alloc(nh.size(), st);
    }
    if (nmaps_regs) hrange.zeros((size_t)roff, ctx->stream, st);
    if (npx) d_histpx.alloc((size_t)npx, st);
    if (reg_close(ctx, "dangx_moments_hist", st, !nh.empty())) return 1;
    m->hrec = std::move(hrec); m->d_hist = std::move(d_hist);
    m->hrange = std::move(hrange); m->d_histpx = std::move(d_histpx);
    m->hpitch = pitch; m->nhist_px = npx; m->nhist_sig = nhs;
    m->sig_table.clear();   // the signal table carries the records of the histograms that read signals
    m->hists = nh;
    m->hbins = nbins; m->hbits = bits;
    m->table.clear();   // the next accumulation uploads the tables
    return 0;
}

// the raw records: a copy on the stream, which the host form waits for
static int hist_get_impl(dangx_ctx* ctx, int reg, void* counts, bool to_host) {
    if (!ctx || !counts || need_live(ctx, "dangx_moments_hist_get") || hist_reg(ctx, reg)) return 1;
    const DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const size_t bytes = sizeof(uint32_t) * (size_t)ctx->dims.npix * dx_hist_words(m->hbins, m->hbits);
    HIPCHK(ctx, hipMemcpyAsync(counts, m->records(m->hists[reg]), bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    if (to_host) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_hist_get_dev(dangx_ctx* ctx, int reg, void* counts_dev) { return hist_get_impl(ctx, reg, counts_dev, false); }

int dangx_moments_hist_get(dangx_ctx* ctx, int reg, void* counts) { return hist_get_impl(ctx, reg, counts, true); }

static int hist_stat_impl(dangx_ctx* ctx, int reg, int stat, int nq, const double* q, double* out, bool to_host) {
    if (!ctx || !out || need_live(ctx, "dangx_moments_hist_stat") || dx_hist_stat_check(ctx, reg, stat, nq, q)) return 1;
    const DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const long long total = (long long)ctx->dims.npix * (stat == 0 ? nq : 1);
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)total)) return 1;
    const auto& h = m->hists[reg];
    HistStatArgs a{};
    a.rec = m->records(h); a.out = ro.dst; a.lo = h.lo; a.hi = h.hi; a.n = ctx->dims.npix;
    a.nbins = m->hbins; a.bits = m->hbits; a.stat = stat; a.nq = stat == 0 ? nq : 0;
    for (int j = 0; j < a.nq; ++j) a.q[j] = q[j];
    const unsigned gx = std::max(1u, std::min(nblocks(a.n), 2048u));
    if (h.kind == DX_HIST_RANGE_PIXEL && stat != 2) {   // quantiles and the mode need the pixel's bounds; N does not
        HistStatPxArgs ap{};
        static_cast<HistStatArgs&>(ap) = a;
        ap.lo_map = m->range_lo(h); ap.hi_map = m->range_hi(h);
        if (!ap.lo_map) return fail(ctx, "posterior moments: dangx_moments_hist_stat: histogram registration " + std::to_string(reg) + " has no range maps");
        hipLaunchKernelGGL(k_hist_stat_px, dim3(gx), dim3(BLOCK), 0, ctx->stream, ap);
    } else {
        hipLaunchKernelGGL(k_hist_stat, dim3(gx), dim3(BLOCK), 0, ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return ro.close(total);
}

// the checks of dangx_moments_hist_range_*: a registration of this context, whatever it has accumulated
static int range_reg(dangx_ctx* ctx, const char* who, int reg) {
    const DxMoments* m = ctx->mom;
    if (reg < 0 || reg >= (int)m->hists.size())
        return fail(ctx, std::string("posterior moments: ") + who + ": histogram registration out of range (" + std::to_string(m->hists.size()) + " registered)");
    return 0;
}

// lo, hi: [npix] of this shard, host or device arrays.  The checksum is taken from the host arrays, or from a staged copy of the
// device arrays (registration is not on the hot path); the library keeps its own copy.
static int range_maps_impl(dangx_ctx* ctx, int reg, const double* lo, const double* hi, bool from_dev) {
    const char* who = "dangx_moments_hist_range_maps";
    if (!ctx || !lo || !hi || reg_open(ctx, who) || range_reg(ctx, who, reg)) return 1;
    DxMoments* m = ctx->mom;
    DxMoments::Hist& h = m->hists[reg];
    if (h.kind != DX_HIST_RANGE_PIXEL)
        return fail(ctx, std::string("posterior moments: ") + who + ": histogram registration " + std::to_string(reg) +
                             " has a global range: it did not declare per-pixel maps (range {-inf, +inf} in dangx_moments_hist)");
    (void)hipSetDevice(ctx->device);
    const size_t np = (size_t)ctx->dims.npix, bytes = sizeof(double) * np;
    std::vector<double> stage;
    const double *hl = lo, *hh = hi;
    if (from_dev) {
        stage.resize(2 * np);
        HIPCHK(ctx, hipMemcpyAsync(stage.data(), lo, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(stage.data() + np, hi, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        hl = stage.data(); hh = stage.data() + np;
    }
    const uint64_t sum = dx_hist_range_checksum(hl, hh, (long long)np);
    double* dlo = m->hrange + h.roff;
    HIPCHK(ctx, hipMemcpyAsync(dlo, hl, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dlo + m->hpitch, hh, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the caller's arrays and the staged copy are free again
    h.have_maps = true;
    h.sum = sum;
    return 0;
}

// the maps of a per-pixel registration as they were handed in; the constants of a global one spread over the shard
static int range_get_impl(dangx_ctx* ctx, int reg, double* lo, double* hi, bool to_dev) {
    const char* who = "dangx_moments_hist_range_get";
    if (!ctx || !lo || !hi || need(ctx) || range_reg(ctx, who, reg)) return 1;
    const DxMoments* m = ctx->mom;
    const DxMoments::Hist& h = m->hists[reg];
    (void)hipSetDevice(ctx->device);
    const size_t np = (size_t)ctx->dims.npix, bytes = sizeof(double) * np;
    if (h.kind != DX_HIST_RANGE_PIXEL) {
        if (!to_dev) {
            std::fill(lo, lo + np, h.lo);
            std::fill(hi, hi + np, h.hi);
            return 0;
        }
        const std::vector<double> vl(np, h.lo), vh(np, h.hi);
        HIPCHK(ctx, hipMemcpyAsync(lo, vl.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(hi, vh.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the staged constants go with this call
        return 0;
    }
    const double *dl = m->range_lo(h), *dh = m->range_hi(h);
    if (!dl)
        return fail(ctx, std::string("posterior moments: ") + who + ": histogram registration " + std::to_string(reg) +
                             (m->holder ? ": section HIST_RANGE(" + std::to_string(reg) + ") was not put into this holder" : " has no range maps yet"));
    const hipMemcpyKind kind = to_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(ctx, hipMemcpyAsync(lo, dl, bytes, kind, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hi, dh, bytes, kind, ctx->stream));
    if (!to_dev) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_hist_range_maps(dangx_ctx* ctx, int reg, const double* lo, const double* hi) { return range_maps_impl(ctx, reg, lo, hi, false); }

int dangx_moments_hist_range_maps_dev(dangx_ctx* ctx, int reg, const double* lo_dev, const double* hi_dev) {
    return range_maps_impl(ctx, reg, lo_dev, hi_dev, true);
}

int dangx_moments_hist_range_get(dangx_ctx* ctx, int reg, double* lo, double* hi) { return range_get_impl(ctx, reg, lo, hi, false); }

int dangx_moments_hist_range_get_dev(dangx_ctx* ctx, int reg, double* lo_dev, double* hi_dev) { return range_get_impl(ctx, reg, lo_dev, hi_dev, true); }

int dangx_moments_hist_stat_dev(dangx_ctx* ctx, int reg, int stat, int nq, const double* q, double* out_dev) {
    return hist_stat_impl(ctx, reg, stat, nq, q, out_dev, false);
}

int dangx_moments_hist_stat(dangx_ctx* ctx, int reg, int stat, int nq, const double* q, double* out) {
    return hist_stat_impl(ctx, reg, stat, nq, q, out, true);
}

int dangx_moments_signals(dangx_ctx* ctx, int nsig, const int32_t* spec) {
    if (reg_open(ctx, "dangx_moments_signals")) return 1;   // its tables come from the descriptors: signals do not depend on the selection
    DxMoments* m = ctx->mom;
    for (const auto& h : m->hists)
        if (h.sig >= 0)
            return fail(ctx, "posterior moments: dangx_moments_signals: histogram registration " + std::to_string(h.id) + " reads signal " +
                                 std::to_string(h.sig) + " of the present list: drop the histograms first (dangx_moments_hist with nreg = 0)");
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
        sg.id = s;
        off += ctx->dims.npix;
        ns.push_back(sg);
    }
    const long long half = off + (off & 1);   // even: the m2 half has the phases of the mean half
    // everything new is allocated before anything old is dropped (reg_close)
    DevBuf<double> sacc;
    DevBuf<SigSeg> d_sig;
    DevStatus st;
    if (!ns.empty()) {
        sacc.zeros(2 * (size_t)half, ctx->stream, st);
        d_sig.alloc(plan.size(), st);
    }
    if (reg_close(ctx, "dangx_moments_signals", st, !ns.empty())) return 1;
    m->sacc = std::move(sacc); m->d_sig = std::move(d_sig); m->sacc_half = half;
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

static int get_signal_impl(dangx_ctx* ctx, int sig, int stat, int ddof, double* out, bool to_host) {
    if (!ctx || !out || signal_get_check(ctx, sig, stat, ddof)) return 1;
    const DxMoments* m = ctx->mom;
    (void)hipSetDevice(ctx->device);
    const long long np = ctx->dims.npix;
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)np)) return 1;
    const auto& s = m->sigs[sig];
    if (finish_plane(ctx, m->mean(s), m->m2(s), stat, (double)(m->count - ddof), ro.dst)) return 1;
    return ro.close(np);
}

int dangx_moments_get_signal_dev(dangx_ctx* ctx, int sig, int stat, int ddof, double* out_dev) {
    return get_signal_impl(ctx, sig, stat, ddof, out_dev, false);
}

int dangx_moments_get_signal(dangx_ctx* ctx, int sig, int stat, int ddof, double* out) {
    return get_signal_impl(ctx, sig, stat, ddof, out, true);
}

int dangx_moments_angles(dangx_ctx* ctx, int nang, const int32_t* spec) {
    if (reg_open(ctx, "dangx_moments_angles")) return 1;   // its tables come from the descriptors: angles do not depend on the selection
    DxMoments* m = ctx->mom;
    const int ncomp = ctx->dims.ncomp;
    int set[MAXC] = {}, global[MAXC] = {}, tcmb[MAXC] = {};
    for (int l = 0; l < ncomp; ++l) {
        set[l] = ctx->comp_set[l] ? 1 : 0;
        global[l] = is_global_type(ctx->desc[l].type) ? 1 : 0;
        tcmb[l] = ctx->desc[l].type == DANGX_TCMB ? 1 : 0;
    }
    const std::string why = dx_angle_check(nang, spec, ncomp, ctx->dims.nbands, ctx->dims.nmaps, set, global, tcmb);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_angles: " + why);
    (void)hipSetDevice(ctx->device);
    bool used[MAXC] = {};
    for (int a = 0; a < nang; ++a) used[spec[2 * a]] = true;
    for (int l = 0; l < ncomp; ++l)   // the chain's maps exist from here on (what dangx_get_amplitude does on first use)
        if (used[l] && ensure_state(ctx, l)) return 1;
    const std::vector<DxAngSeg> plan = dx_angle_plan(nang, spec, ncomp, ctx->dims.nbands);
    // accumulators: both planes of an angle at the 16-byte phase of the component's Q plane, so that the streams line up
    std::vector<DxMoments::Ang> na;
    long long off = 0;
    for (int a = 0; a < nang; ++a) {
        DxMoments::Ang ag{spec[2 * a], spec[2 * a + 1], 0};
        const double* plane = ctx->amp[ag.comp] + (long long)ctx->dims.npix;
        const long long phase = (long long)((reinterpret_cast<uintptr_t>(plane) >> 3) & 1);
        if ((off & 1) != phase) ++off;
        ag.off = off;
        ag.id = a;
        off += ctx->dims.npix;
        na.push_back(ag);
    }
    const long long half = off + (off & 1);   // even: the Sbar half has the phases of the Cbar half
    // everything new is allocated before anything old is dropped (reg_close)
    DevBuf<double> aacc;
    DevBuf<AngSeg> d_ang;
    DevStatus st;
    if (!na.empty()) {
        aacc.zeros(2 * (size_t)half, ctx->stream, st);
        d_ang.alloc(plan.size(), st);
    }
    if (reg_close(ctx, "dangx_moments_angles", st, !na.empty())) return 1;
    m->aacc = std::move(aacc); m->d_ang = std::move(d_ang); m->aacc_half = half;
    m->angs = na;
    m->ang_plan = plan;
    m->ang_table.clear();   // the next accumulation uploads the table
    for (int l = 0; l < MAXC; ++l) {
        m->ang_used[l] = l < ncomp && used[l];
        m->ang_type[l] = m->ang_used[l] ? ctx->desc[l].type : 0;
        m->ang_nind[l] = m->ang_used[l] ? ctx->desc[l].nindices : 0;
    }
    return 0;
}

static int get_angle_impl(dangx_ctx* ctx, int ang, int stat, double* out, bool to_host) {
    if (!ctx || !out || need_live(ctx, "dangx_moments_get_angle")) return 1;
    const DxMoments* m = ctx->mom;
    if (ang < 0 || ang >= (int)m->angs.size())
        return fail(ctx, "posterior moments: angle index out of range (" + std::to_string(m->angs.size()) + " angles registered)");
    const std::string why = dx_angle_stat_check(stat, 1);
    if (!why.empty()) return fail(ctx, "posterior moments: " + why);
    if (count_check(ctx, nullptr, 0)) return 1;
    (void)hipSetDevice(ctx->device);
    const long long np = ctx->dims.npix;
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)np)) return 1;
    const auto& a = m->angs[ang];
    const unsigned gx = std::max(1u, std::min(nblocks(np), 1024u));
    hipLaunchKernelGGL(k_angle_finish, dim3(gx), dim3(BLOCK), 0, ctx->stream, (const double*)m->angC(a), (const double*)m->angS(a), ro.dst, np, stat);
    HIPCHK(ctx, hipGetLastError());
    return ro.close(np);
}

int dangx_moments_get_angle_dev(dangx_ctx* ctx, int ang, int stat, double* out_dev) { return get_angle_impl(ctx, ang, stat, out_dev, false); }

int dangx_moments_get_angle(dangx_ctx* ctx, int ang, int stat, double* out) { return get_angle_impl(ctx, ang, stat, out, true); }

int dangx_moments_fit(dangx_ctx* ctx, int nfit, const int32_t* spec) {
    if (reg_open(ctx, "dangx_moments_fit")) return 1;   // every component enters the residual: nothing to look up in the selection
    DxMoments* m = ctx->mom;
    const std::string why = dx_fit_check(nfit, spec, ctx->dims.nbands, ctx->dims.nmaps);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_fit: " + why);
    (void)hipSetDevice(ctx->device);
    const std::vector<DxFitSeg> plan = dx_fit_plan(nfit, spec, ctx->dims.nbands);
    std::vector<DxMoments::Fit> nf;
    for (int i = 0; i < nfit; ++i) nf.push_back(DxMoments::Fit{spec[3 * i], spec[3 * i + 1], spec[3 * i + 2], (long long)i * ctx->dims.npix, i});
    const long long half = (long long)nfit * ctx->dims.npix;
    // everything new is allocated before anything old is dropped (reg_close)
    DevBuf<double> facc;
    DevBuf<FitSeg> d_fit;
    DevStatus st;
    if (!nf.empty()) {
        facc.zeros(2 * (size_t)half, ctx->stream, st);
        d_fit.alloc(plan.size(), st);
    }
    if (reg_close(ctx, "dangx_moments_fit", st, !nf.empty())) return 1;
    m->facc = std::move(facc); m->d_fit = std::move(d_fit); m->facc_half = half;
    m->fits = nf;
    m->fit_plan = plan;
    m->fit_table.clear();   // the next accumulation uploads the table
    return 0;
}

static int get_fit_impl(dangx_ctx* ctx, int item, int stat, int ddof, double* out, bool to_host) {
    if (!ctx || !out || need_live(ctx, "dangx_moments_get_fit")) return 1;
    const DxMoments* m = ctx->mom;
    if (item < 0 || item >= (int)m->fits.size())
        return fail(ctx, "posterior moments: fit item out of range (" + std::to_string(m->fits.size()) + " fit items registered)");
    if (stat != 0 && stat != 1) return fail(ctx, "posterior moments: the stat of a fit item must be 0 (mean) or 1 (standard deviation)");
    if (count_check(ctx, stat == 1 ? "standard deviation" : nullptr, ddof)) return 1;
    (void)hipSetDevice(ctx->device);
    const long long np = ctx->dims.npix;
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)np)) return 1;
    const auto& f = m->fits[item];
    if (finish_plane(ctx, m->mean(f), m->m2(f), stat, (double)(m->count - ddof), ro.dst)) return 1;
    return ro.close(np);
}

int dangx_moments_get_fit_dev(dangx_ctx* ctx, int item, int stat, int ddof, double* out_dev) {
    return get_fit_impl(ctx, item, stat, ddof, out_dev, false);
}

int dangx_moments_get_fit(dangx_ctx* ctx, int item, int stat, int ddof, double* out) {
    return get_fit_impl(ctx, item, stat, ddof, out, true);
}

int dangx_moments_batches(dangx_ctx* ctx, int nreg, const int32_t* planes, int nbatch, int64_t batch_len) {
    RegTables tab;
    if (reg_open(ctx, "dangx_moments_batches", &tab)) return 1;
    DxMoments* m = ctx->mom;
    const std::string why = dx_batches_check(nreg, planes, nbatch, batch_len, ctx->dims.ncomp, ctx->dims.nmaps, m->sel, tab.nind, tab.global);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_batches: " + why);
    const long long pitch = ctx->dims.npix + (ctx->dims.npix & 1);   // even: every plane of a registration at the phase of its first
    std::vector<DxMoments::Batch> nb;
    long long off = 0;
    for (int r = 0; r < nreg; ++r) {
        const int seg = m->find_seg(planes[3 * r], planes[3 * r + 1], planes[3 * r + 2]);
        if (seg < 0) return fail(ctx, "posterior moments: dangx_moments_batches: registration " + std::to_string(r) + ": a plane that is not selected");
        if ((off & 1) != (m->segs[seg].off & 1)) ++off;
        nb.push_back(DxMoments::Batch{seg, off, r});
        off += 2LL * nbatch * pitch;
    }
    (void)hipSetDevice(ctx->device);
    // everything new is allocated before anything old is dropped (reg_close)
    DevBuf<double> bacc;
    DevBuf<MomSeg> d_batch;
    DevStatus st;
    if (!nb.empty()) {
        bacc.zeros((size_t)off, ctx->stream, st);
        d_batch.alloc(nb.size() * (size_t)nbatch, st);
    }
    if (reg_close(ctx, "dangx_moments_batches", st, !nb.empty())) return 1;
    m->bacc = std::move(bacc); m->d_batch = std::move(d_batch);
    m->batches = nb;
    m->nbatch = nb.empty() ? 0 : nbatch;
    m->batch_len = nb.empty() ? 0 : (long long)batch_len;
    m->bpitch = pitch;
    m->table.clear();   // the next accumulation uploads the tables
    return 0;
}

static int batches_need(dangx_ctx* ctx, int reg) {
    if (need(ctx)) return 1;
    const DxMoments* m = ctx->mom;
    if (m->batches.empty()) return fail(ctx, "posterior moments: no batches are registered (dangx_moments_batches was not called)");
    if (reg < 0 || reg >= (int)m->batches.size())
        return fail(ctx, "posterior moments: batch registration out of range (" + std::to_string(m->batches.size()) + " registered)");
    return 0;
}

int dangx_moments_batches_info(dangx_ctx* ctx, int64_t* batch_len, int32_t* nfull, int64_t* partial) {
    if (!ctx || batches_need(ctx, 0)) return 1;
    const DxMoments* m = ctx->mom;
    const DxBatchPos p = dx_batches_pos(m->count, m->batch_len);
    if (batch_len) *batch_len = p.L;
    if (nfull) *nfull = p.nfull;
    if (partial) *partial = p.partial;
    return 0;
}

static int batches_get_impl(dangx_ctx* ctx, int reg, int stat, int first, int ddof, double* out, bool to_host) {
    if (!ctx || !out || need_live(ctx, "dangx_moments_batches_get") || batches_need(ctx, reg)) return 1;
    const DxMoments* m = ctx->mom;
    if (count_check(ctx, nullptr, 0)) return 1;
    const DxBatchPos p = dx_batches_pos(m->count, m->batch_len);
    const std::string why = dx_batches_stat_check(stat, first, ddof, p.L, p.nfull, p.partial);
    if (!why.empty()) return fail(ctx, "posterior moments: dangx_moments_batches_get: " + why);
    (void)hipSetDevice(ctx->device);
    const long long n = ctx->dims.npix;
    ReadOut ro{ctx, out, to_host};
    if (ro.open(sizeof(double) * (size_t)n)) return 1;
    BatchStatArgs a{};
    a.base = m->bmean(m->batches[reg], 0); a.out = ro.dst; a.pitch = m->bpitch; a.n = n;
    a.par = dx_batches_par(stat, first, ddof, p.L, p.nfull, p.partial);
    hipLaunchKernelGGL(k_batches_stat, dim3(m->grid_for((n + 1) / 2, 1)), dim3(BLOCK), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return ro.close(n);
}

int dangx_moments_batches_get_dev(dangx_ctx* ctx, int reg, int stat, int first, int ddof, double* out_dev) {
    return batches_get_impl(ctx, reg, stat, first, ddof, out_dev, false);
}

int dangx_moments_batches_get(dangx_ctx* ctx, int reg, int stat, int first, int ddof, double* out) {
    return batches_get_impl(ctx, reg, stat, first, ddof, out, true);
}

// one slot's two planes as they are: copies on the stream, which the host form waits for
static int batches_raw_impl(dangx_ctx* ctx, int reg, int batch, double* mean_out, double* m2_out, bool to_host) {
    if (!ctx || need_live(ctx, "dangx_moments_batches_raw") || batches_need(ctx, reg)) return 1;
    const DxMoments* m = ctx->mom;
    if (batch < 0 || batch >= m->nbatch)
        return fail(ctx, "posterior moments: dangx_moments_batches_raw: batch out of range (nbatch = " + std::to_string(m->nbatch) + ")");
    (void)hipSetDevice(ctx->device);
    const size_t bytes = sizeof(double) * (size_t)ctx->dims.npix;
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const auto& r = m->batches[reg];
    if (mean_out) HIPCHK(ctx, hipMemcpyAsync(mean_out, m->bmean(r, batch), bytes, kind, ctx->stream));
    if (m2_out) HIPCHK(ctx, hipMemcpyAsync(m2_out, m->bm2(r, batch), bytes, kind, ctx->stream));
    if (to_host) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int dangx_moments_batches_raw_dev(dangx_ctx* ctx, int reg, int batch, double* mean_out_dev, double* m2_out_dev) {
    return batches_raw_impl(ctx, reg, batch, mean_out_dev, m2_out_dev, false);
}

int dangx_moments_batches_raw(dangx_ctx* ctx, int reg, int batch, double* mean_out, double* m2_out) {
    return batches_raw_impl(ctx, reg, batch, mean_out, m2_out, true);
}

}  // extern "C"

// ---- sections: one part of the accumulator state in its packed layout (dx_section_host.h), read or written by copies on the
// context's stream, and holders (dangx_moments_begin_like), which keep sections put into them for dangx_chains_*

static DxSecReg section_reg(const dangx_ctx* ctx, const DxMoments* m) {
    DxSecReg r;
    r.npix = ctx->dims.npix; r.pix0 = ctx->dims.pix0; r.nmaps = ctx->dims.nmaps;
    for (int l = 0; l < ctx->dims.ncomp; ++l) { r.sel.push_back(m->sel[l]); r.type.push_back(m->type[l]); r.nind.push_back(m->nind[l]); }
    r.lag1 = m->lag1 ? 1 : 0;
    auto plane = [&](std::vector<int32_t>& v, int seg) { const auto& s = m->segs[seg]; v.push_back(s.comp); v.push_back(s.what); v.push_back(s.plane); };
    for (const auto& p : m->pairs) { plane(r.pairs, p.a); plane(r.pairs, p.b); }
    for (const auto& h : m->hists) {
        if (h.sig >= 0) { r.hist_planes.push_back(h.sig); r.hist_planes.push_back(DX_HIST_SIGNAL); r.hist_planes.push_back(0); }
        else plane(r.hist_planes, h.seg);
        r.hist_range.push_back(h.lo); r.hist_range.push_back(h.hi);
        r.hist_kind.push_back(h.kind); r.hist_sum.push_back(h.sum);
    }
    r.nbins = m->hbins; r.bits = m->hbits;
    for (const auto& s : m->sigs) { r.signals.push_back(s.comp); r.signals.push_back(s.band); r.signals.push_back(s.kind); }
    for (const auto& a : m->angs) { r.angles.push_back(a.comp); r.angles.push_back(a.band); }
    for (const auto& f : m->fits) { r.fit.push_back(f.what); r.fit.push_back(f.band); r.fit.push_back(f.plane); }
    for (const auto& b : m->batches) plane(r.batch_planes, b.seg);
    r.nbatch = m->nbatch;
    return r;
}

namespace {

struct SecRun { void* dev; void* host; long long off, bytes; };   // a run of the payload at `off`: in HBM (dev) or a host row of the state

struct SecShape {          // a section of this context's registration
    long long bytes = 0;   // the payload
    int nsel = 0;          // PLANES: selected planes
    unsigned planes = 0;
    bool global = false;   // PLANES: the host rows of a template / monopole / hi_fit member
};

std::string section_name(int family, int a, int b) {
    std::string s = dx_section_family_name(family);
    if (family == DX_SEC_PLANES) s += "(" + std::to_string(a) + ", " + std::to_string(b) + ")";
    else if (family != DX_SEC_HEAD) s += "(" + std::to_string(a) + ")";
    return s;
}

int section_shape(dangx_ctx* ctx, const char* who, int family, int a, int b, SecShape& sh) {
    if (need(ctx)) return 1;
    const DxMoments* m = ctx->mom;
    const long long np = ctx->dims.npix;
    auto range = [&](size_t n, const char* noun) {
        if (a >= 0 && a < (int)n) return 0;
        return fail(ctx, std::string("posterior moments: ") + who + ": " + noun + " out of range (" + std::to_string(n) + " registered)");
    };
    switch (family) {
    case DX_SEC_HEAD: sh.bytes = DX_SEC_HEAD_BYTES; return 0;
    case DX_SEC_PLANES: {
        if (a < 0 || a >= ctx->dims.ncomp) return fail(ctx, std::string("posterior moments: ") + who + ": component index out of range");
        if (b < 0 || b > DANGX_MAX_IND) return fail(ctx, std::string("posterior moments: ") + who + ": what must be 0 (amplitude) or 1 + index number");
        sh.planes = (unsigned)(m->sel[a] >> (b == 0 ? 0 : 3 + 3 * (b - 1))) & 7u;
        sh.nsel = __builtin_popcount(sh.planes);
        if (!sh.nsel) return fail(ctx, std::string("posterior moments: ") + who + ": nothing selected for this component and what");
        sh.global = b == 0 && is_global_type(m->type[a]);
        sh.bytes = dx_section_planes_bytes(sh.global ? ctx->dims.nbands : np, sh.nsel, m->lag1);
        return 0;
    }
    case DX_SEC_PAIR: if (range(m->pairs.size(), "pair index")) return 1; sh.bytes = dx_section_pair_bytes(np); return 0;
    case DX_SEC_HIST: if (range(m->hists.size(), "histogram registration")) return 1; sh.bytes = dx_section_hist_bytes(np, m->hbins, m->hbits); return 0;
    case DX_SEC_SIGNAL: if (range(m->sigs.size(), "signal index")) return 1; sh.bytes = dx_section_signal_bytes(np); return 0;
    case DX_SEC_BATCHES: if (range(m->batches.size(), "batch registration")) return 1; sh.bytes = dx_section_batches_bytes(np, m->nbatch); return 0;
    case DX_SEC_HIST_RANGE:
        if (range(m->hists.size(), "histogram registration")) return 1;
        if (m->hists[a].kind != DX_HIST_RANGE_PIXEL)
            return fail(ctx, std::string("posterior moments: ") + who + ": section " + section_name(family, a, b) + ": histogram registration " +
                                 std::to_string(a) + " has a global range and no range maps");
        sh.bytes = dx_section_hist_range_bytes(np);
        return 0;
    case DX_SEC_ANGLE:
        if (m->angs.empty()) break;   // a context without angles has the families it always had
        if (range(m->angs.size(), "angle index")) return 1;
        sh.bytes = dx_section_angle_bytes(np);
        return 0;
    case DX_SEC_FIT:
        if (m->fits.empty()) break;   // likewise
        if (range(m->fits.size(), "fit item")) return 1;
        sh.bytes = dx_section_fit_bytes(np);
        return 0;
    }
    return fail(ctx, std::string("posterior moments: ") + who + ": family must be 0 (HEAD) .. 6 (HIST_RANGE), or 7 (ANGLE) where angles are registered, or 8 (FIT) where fit items are");
}

// a holder's buffer for a section of `bytes` payload bytes, and its planes entered into the tables
int holder_take(dangx_ctx* ctx, int family, int a, int b, const SecShape& sh, long long bytes) {
    DxMoments* m = ctx->mom;
    // batches at the pitch of a live context (the kernels over several chains take ONE pitch, chain 0's), everything else packed
    const size_t want = (size_t)dx_section_round256(family == DX_SEC_BATCHES ? 16LL * m->nbatch * m->bpitch : bytes);
    DxMoments::Held* h = nullptr;
    for (auto& x : m->held)
        if (x.family == family && x.a == a && x.b == b) h = &x;
    if (!h || h->bytes != want) {
        DevBuf<unsigned char> nb;
        DevStatus st;
        nb.alloc(want, st);
        if (!st.ok()) return st.fail(ctx, "dangx_moments_section_put: ");
        if (h) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // nothing may still read the buffer that goes
            h->buf = std::move(nb);
            h->bytes = want;
        } else {
            m->held.push_back(DxMoments::Held{family, a, b, std::move(nb), want});
            h = &m->held.back();
        }
    }
    const long long np = ctx->dims.npix;
    double* base = reinterpret_cast<double*>(h->buf.p);
    switch (family) {
    case DX_SEC_PLANES: {
        const bool lag = bytes == dx_section_planes_bytes(np, sh.nsel, 1);
        int r = 0;
        for (int k = 0; k < ctx->dims.nmaps; ++k) {
            if (!((sh.planes >> k) & 1u)) continue;
            DxMoments::HeldSeg& t = m->h_seg[m->find_seg(a, b, k)];
            t.mean = base + (long long)r * np;
            t.m2 = base + (long long)(sh.nsel + r) * np;
            t.prev = lag ? base + (long long)(2 * sh.nsel + r) * np : nullptr;
            t.first = lag ? base + (long long)(3 * sh.nsel + r) * np : nullptr;
            t.P = lag ? base + (long long)(4 * sh.nsel + r) * np : nullptr;
            ++r;
        }
        break;
    }
    case DX_SEC_PAIR: m->h_pair[a] = base; break;
    case DX_SEC_HIST: m->h_hist[a] = reinterpret_cast<uint32_t*>(h->buf.p); break;
    case DX_SEC_SIGNAL: m->h_sig[a].mean = base; m->h_sig[a].m2 = base + np; break;
    case DX_SEC_BATCHES: m->h_batch[a] = base; break;
    case DX_SEC_HIST_RANGE: m->h_range[a] = base; break;
    case DX_SEC_ANGLE: m->h_ang[a].mean = base; m->h_ang[a].m2 = base + np; break;
    case DX_SEC_FIT: m->h_fit[a].mean = base; m->h_fit[a].m2 = base + np; break;
    }
    return 0;
}

// the runs of a section's payload where the context keeps them; nparts: the parts of a PLANES payload that travel
int section_runs(dangx_ctx* ctx, const char* who, int family, int a, int b, const SecShape& sh, int nparts, bool put, std::vector<SecRun>& runs) {
    DxMoments* m = ctx->mom;
    const long long np = ctx->dims.npix, plane = 8 * np;
    auto add = [&](void* dev, long long off, long long bytes) { runs.push_back(SecRun{dev, nullptr, off, bytes}); };
    switch (family) {
    case DX_SEC_PLANES: {
        int r = 0;
        for (int k = 0; k < ctx->dims.nmaps; ++k) {
            if (!((sh.planes >> k) & 1u)) continue;
            if (sh.global) {
                double* rows[5] = {m->tm_mean[a][k], m->tm_m2[a][k], m->tm_prev[a][k], m->tm_first[a][k], m->tm_P[a][k]};
                const long long row = 8LL * ctx->dims.nbands;
                for (int p = 0; p < nparts; ++p) runs.push_back(SecRun{nullptr, rows[p], ((long long)p * sh.nsel + r) * row, row});
            } else {
                const auto& s = m->segs[m->find_seg(a, b, k)];
                double* part[5] = {m->mean(s), m->m2(s), nparts > 2 ? m->prev(s) : nullptr, nparts > 2 ? m->first(s) : nullptr, nparts > 2 ? m->P(s) : nullptr};
                for (int p = 0; p < nparts; ++p) add(part[p], ((long long)p * sh.nsel + r) * plane, plane);
            }
            ++r;
        }
        break;
    }
    case DX_SEC_PAIR: add(m->C(m->pairs[a]), 0, plane); break;
    case DX_SEC_HIST: add(m->records(m->hists[a]), 0, sh.bytes); break;
    case DX_SEC_SIGNAL: add(m->mean(m->sigs[a]), 0, plane); add(m->m2(m->sigs[a]), plane, plane); break;
    case DX_SEC_BATCHES:
        for (int t = 0; t < m->nbatch; ++t) {
            add(m->bmean(m->batches[a], t), 2LL * t * plane, plane);
            add(m->bm2(m->batches[a], t), (2LL * t + 1) * plane, plane);
        }
        break;
    case DX_SEC_HIST_RANGE:
        if (!m->holder && !m->hists[a].have_maps)
            return fail(ctx, std::string("posterior moments: ") + who + ": section " + section_name(family, a, b) + ": histogram registration " +
                                 std::to_string(a) + " has no range maps yet (dangx_moments_hist_range_maps)");
        add(m->range_lo(m->hists[a]), 0, plane); add(m->range_hi(m->hists[a]), plane, plane);
        break;
    case DX_SEC_ANGLE: add(m->angC(m->angs[a]), 0, plane); add(m->angS(m->angs[a]), plane, plane); break;
    case DX_SEC_FIT: add(m->mean(m->fits[a]), 0, plane); add(m->m2(m->fits[a]), plane, plane); break;
    }
    bool missing = !put && m->holder && family == DX_SEC_PLANES && sh.global && !m->h_rows[a];
    for (const SecRun& r : runs) missing = missing || (!r.dev && !r.host);
    if (missing)
            return fail(ctx, std::string("posterior moments: ") + who + ": section " + section_name(family, a, b) + " was not put into this holder");
    return 0;
}

int section_head_own(dangx_ctx* ctx, DxSecHead& h) {
    const DxMoments* m = ctx->mom;
    h = dx_section_head(section_reg(ctx, m), m->count, m->batch_len);
    return 0;
}

int section_move(dangx_ctx* ctx, const char* who, int family, int a, int b, void* user, long long bytes, bool put, bool user_dev) {
    if (!ctx || !user) return 1;
    SecShape sh;
    if (section_shape(ctx, who, family, a, b, sh)) return 1;
    DxMoments* m = ctx->mom;
    const std::string name = section_name(family, a, b);
    int nparts = (int)dx_section_planes_parts(m->lag1);
    // a holder takes the first two parts (mean, m2) of a PLANES section alone: what R-hat and the pooled moments need
    const bool short_put = put && m->holder && family == DX_SEC_PLANES && !sh.global && m->lag1 && bytes == dx_section_planes_bytes(ctx->dims.npix, sh.nsel, 0);
    if (short_put) nparts = 2;
    else if (bytes != sh.bytes)
        return fail(ctx, std::string("posterior moments: ") + who + ": section " + name + " is " + std::to_string(sh.bytes) + " bytes, not " + std::to_string(bytes));
    if (family == DX_SEC_HEAD) {
        if (user_dev) return fail(ctx, std::string("posterior moments: ") + who + ": HEAD is a host section (use the host form)");
        DxSecHead own;
        section_head_own(ctx, own);
        if (!put) {
            if (m->holder && !m->head_put) return fail(ctx, std::string("posterior moments: ") + who + ": section HEAD was not put into this holder");
            dx_section_head_pack(own, static_cast<unsigned char*>(user));
            return 0;
        }
        DxSecHead got;
        std::string why = dx_section_head_unpack(static_cast<const unsigned char*>(user), (size_t)bytes, got);
        if (why.empty()) {
            why = dx_section_head_diff(got, own);
            if (!why.empty()) why = "HEAD does not fit this context's registration: " + why;
        }
        if (why.empty() && !m->hists.empty() && got.count > 0) why = dx_hist_limit_check(got.count, m->hbits);
        if (!why.empty()) return fail(ctx, std::string("posterior moments: ") + who + ": " + why);
        m->count = got.count;
        if (!m->batches.empty()) m->batch_len = got.batch_len;
        if (m->holder) m->head_put = true;
        return 0;
    }
    (void)hipSetDevice(ctx->device);
    if (put && family == DX_SEC_HIST_RANGE) {   // the maps put are the registration's: checked before anything is written
        const size_t np = (size_t)ctx->dims.npix;
        std::vector<double> stage;
        const double* v = static_cast<const double*>(user);
        if (user_dev) {
            stage.resize(2 * np);
            HIPCHK(ctx, hipMemcpyAsync(stage.data(), user, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            v = stage.data();
        }
        if (!m->holder && !m->hists[a].have_maps)
            return fail(ctx, std::string("posterior moments: ") + who + ": section " + name + ": histogram registration " + std::to_string(a) +
                                 " has no range maps yet (dangx_moments_hist_range_maps first: a put does not register them)");
        if (dx_hist_range_checksum(v, v + np, (long long)np) != m->hists[a].sum)
            return fail(ctx, std::string("posterior moments: ") + who + ": section " + name + ": the checksum of these maps is not that of histogram registration " +
                                 std::to_string(a));
    }
    if (put && m->holder && !sh.global && holder_take(ctx, family, a, b, sh, bytes)) return 1;
    std::vector<SecRun> runs;
    if (section_runs(ctx, who, family, a, b, sh, nparts, put, runs)) return 1;
    char* u = static_cast<char*>(user);
    bool wait = !user_dev;
    for (const SecRun& r : runs) {
        if (r.host && !user_dev) {   // host rows and a host array: no device involved
            if (put) std::memcpy(r.host, u + r.off, (size_t)r.bytes);
            else std::memcpy(u + r.off, r.host, (size_t)r.bytes);
            continue;
        }
        void* mine = r.host ? r.host : r.dev;
        const hipMemcpyKind kind = r.host ? (put ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice)
                                          : user_dev ? hipMemcpyDeviceToDevice : put ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        if (put) HIPCHK(ctx, hipMemcpyAsync(mine, u + r.off, (size_t)r.bytes, kind, ctx->stream));
        else HIPCHK(ctx, hipMemcpyAsync(u + r.off, mine, (size_t)r.bytes, kind, ctx->stream));
        wait = wait || r.host;   // the host rows are the state itself: the copy is over when the call returns
    }
    if (wait) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (put && m->holder && sh.global) m->h_rows[a] = true;
    return 0;
}

}  // namespace

extern "C" {

int dangx_moments_section_bytes(dangx_ctx* ctx, int family, int a, int b, int64_t* bytes) {
    if (!ctx || !bytes) return 1;
    SecShape sh;
    if (section_shape(ctx, "dangx_moments_section_bytes", family, a, b, sh)) return 1;
    *bytes = sh.bytes;
    return 0;
}

int dangx_moments_section_get(dangx_ctx* ctx, int family, int a, int b, void* out, int64_t bytes) {
    return section_move(ctx, "dangx_moments_section_get", family, a, b, out, bytes, false, false);
}

int dangx_moments_section_get_dev(dangx_ctx* ctx, int family, int a, int b, void* out_dev, int64_t bytes) {
    return section_move(ctx, "dangx_moments_section_get_dev", family, a, b, out_dev, bytes, false, true);
}

int dangx_moments_section_put(dangx_ctx* ctx, int family, int a, int b, const void* in, int64_t bytes) {
    return section_move(ctx, "dangx_moments_section_put", family, a, b, const_cast<void*>(in), bytes, true, false);
}

int dangx_moments_section_put_dev(dangx_ctx* ctx, int family, int a, int b, const void* in_dev, int64_t bytes) {
    return section_move(ctx, "dangx_moments_section_put_dev", family, a, b, const_cast<void*>(in_dev), bytes, true, true);
}

int dangx_moments_begin_like(dangx_ctx* ctx, dangx_ctx* like) {
    if (!ctx || !like) return 1;
    if (ctx == like) return fail(ctx, "posterior moments: dangx_moments_begin_like: a context cannot be a holder like itself");
    if (!like->mom) return fail(ctx, "posterior moments: dangx_moments_begin_like: dangx_moments_begin was not called on the other context");
    const DxMoments* o = like->mom;
    if (ctx->dims.npix != like->dims.npix || ctx->dims.pix0 != like->dims.pix0 || ctx->dims.nmaps != like->dims.nmaps ||
        ctx->dims.ncomp != like->dims.ncomp || ctx->dims.nbands != like->dims.nbands)
        return fail(ctx, "posterior moments: dangx_moments_begin_like: the contexts differ in npix / pix0 / nmaps / ncomp / nbands");
    for (int l = 0; l < ctx->dims.ncomp; ++l)
        if ((o->sel[l] || o->sig_used[l] || o->ang_used[l]) && (!ctx->comp_set[l] || ctx->desc[l].type != like->desc[l].type || ctx->desc[l].nindices != like->desc[l].nindices))
            return fail(ctx, "posterior moments: dangx_moments_begin_like: component " + std::to_string(l) + " is not the other context's");
    (void)hipSetDevice(ctx->device);
    if (ctx->mom) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // no launch may still read what is dropped
    std::unique_ptr<DxMoments> m(new DxMoments());
    m->holder = true;
    std::memcpy(m->sel, o->sel, sizeof m->sel); std::memcpy(m->type, o->type, sizeof m->type); std::memcpy(m->nind, o->nind, sizeof m->nind);
    m->segs = o->segs; m->grid_target = o->grid_target;
    m->lag1 = o->lag1; m->pairs = o->pairs;
    m->hists = o->hists; m->hbins = o->hbins; m->hbits = o->hbits;   // range kind and checksum included; the maps come by a put of HIST_RANGE
    for (auto& h : m->hists) { h.have_maps = false; h.roff = 0; }
    m->nhist_px = o->nhist_px; m->nhist_sig = o->nhist_sig; m->hpitch = ctx->dims.npix;            // a section's payload is packed
    m->sigs = o->sigs; m->sig_plan = o->sig_plan;
    std::memcpy(m->sig_type, o->sig_type, sizeof m->sig_type); std::memcpy(m->sig_nind, o->sig_nind, sizeof m->sig_nind);
    std::memcpy(m->sig_used, o->sig_used, sizeof m->sig_used);
    m->angs = o->angs; m->ang_plan = o->ang_plan;
    std::memcpy(m->ang_type, o->ang_type, sizeof m->ang_type); std::memcpy(m->ang_nind, o->ang_nind, sizeof m->ang_nind);
    std::memcpy(m->ang_used, o->ang_used, sizeof m->ang_used);
    m->fits = o->fits; m->fit_plan = o->fit_plan;
    m->batches = o->batches; m->nbatch = o->nbatch; m->batch_len = o->batch_len; m->bpitch = o->bpitch;
    m->h_seg.resize(m->segs.size()); m->h_pair.assign(m->pairs.size(), nullptr); m->h_hist.assign(m->hists.size(), nullptr);
    m->h_range.assign(m->hists.size(), nullptr);
    m->h_sig.resize(m->sigs.size()); m->h_batch.assign(m->batches.size(), nullptr); m->h_ang.resize(m->angs.size());
    m->h_fit.resize(m->fits.size());
    dx_moments_free(ctx);   // whatever the context held or accumulated goes
    ctx->mom = m.release();
    return 0;
}

int dangx_moments_held_bytes(dangx_ctx* ctx, int64_t* bytes) {
    if (!ctx || !bytes || need(ctx)) return 1;
    const DxMoments* m = ctx->mom;
    long long total = 0;
    for (const auto& h : m->held) total += (long long)h.bytes;
    *bytes = total;   // a live context holds nothing: its accumulators are its own
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
