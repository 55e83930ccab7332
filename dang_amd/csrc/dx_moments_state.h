// dx_moments_state.h -- host: the state behind dangx_moments_* (dangx_moments.hip, which writes it) and dangx_chains_*
// (dangx_chains.hip, which only reads it): the registrations, the device allocations that hold their accumulators and the one
// vocabulary for the addresses inside them, plus the helpers every read-out shares.
#pragma once
#include "dx_host.h"
#include "dx_signal_host.h"
#include "dx_angle_host.h"
#include "dx_fit_host.h"

#include <cstdint>
#include <utility>

// ---- the tables the accumulation kernels read

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

struct HistPxSeg {        // a registered histogram with per-pixel ranges: HistSeg with the two range maps in place of the constants
    const double* x;
    uint32_t* rec;
    const double* lo;     // [n], the library's copy, at the 16-byte phase of the segment's accumulators (Seg::off & 1: the phase
                          // the chain's plane had at dangx_moments_begin, which lays the accumulators out by it)
    const double* hi;
    long long n;
    int nbins, bits;
};

struct SigBand {          // one band of a signal segment: the accumulators of its outputs (slot 0..2: T, or Q, U, P), null = not wanted
    double* mean[3];
    double* m2[3];
    int band;
    unsigned want;        // bit o: output slot o is registered
};

// The histograms that read the outputs of one band of a signal segment (k_moments_signal<BP, true> alone looks here; a table of
// its own behind the bands, so that SigBand and what the plain form reads stay laid out as they were): per output slot the
// records, null = none, and the range -- the maps lo[o], hi[o] at the phase of the output's accumulators, or with lo[o] == null
// the two numbers glo[o], ghi[o]
struct SigHistBand {
    uint32_t* rec[3];
    const double* lo[3];
    const double* hi[3];
    double glo[3], ghi[3];
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
    SigHistBand hb[DX_SIG_SEG_BANDS];   // by band, as b
    int hbins, hbits;     // the context's nbins and bits, for the outputs with a histogram
};

struct AngBand {          // one band of an angle segment: the two accumulators of the angle registered there
    double* C;
    double* S;
    int band;
    int pad_;
};

struct AngSeg {           // a component with up to DX_ANG_SEG_BANDS bands; the chain's planes resolved at accumulate time
    const double* amp;    // the component's [nmaps][npix]: what the table is compared by
    const double* idx;    // the component's [nind][nmaps][npix]
    // src[k][0..2]: the amplitude and the two index planes of plane Q (k = 0) and U (k = 1).  An index plane the component does
    // not have points at the amplitude plane, which IS read: the load hits the cache and its value is never used
    const double* src[2][3];
    long long n;
    int comp, nb;
    int vec, nind;        // as SigSeg's
    AngBand b[DX_ANG_SEG_BANDS];
};

struct FitSeg {           // a plane with fit items (dx_fit_host.h): the accumulators of its chi^2 map and of its bands' residuals, null = not registered
    double* chi_mean;
    double* chi_m2;
    double* rmean[MAXB];  // by band
    double* rm2[MAXB];
    int plane;            // 0-based
    int pad_;
};

// ---- device memory that belongs to its holder: freed when the holder goes, handed on by move

struct DevStatus {        // the first HIP call of a sequence that failed (`what` names it); later calls of the sequence do nothing
    hipError_t e = hipSuccess;
    const char* what = "";
    bool ok() const { return e == hipSuccess; }
    void sync(hipStream_t s) {
        if (!ok()) return;
        what = "hipStreamSynchronize";
        e = hipStreamSynchronize(s);
    }
    int fail(dangx_ctx* ctx, const char* where) const {   // where: "" or "dangx_moments_xyz: "
        ctx->err = std::string("posterior moments: ") + where + what + ": " + hipGetErrorString(e);
        return 1;
    }
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }   // what this held dies with o
    operator T*() const { return p; }
    void alloc(size_t count, DevStatus& st) {
        if (!st.ok()) return;
        st.what = "hipMalloc";
        st.e = hipMalloc(&p, sizeof(T) * count);
    }
    void zeros(size_t count, hipStream_t s, DevStatus& st) {   // the fill is enqueued on s: the caller waits (DevStatus::sync)
        alloc(count, st);
        if (!st.ok()) return;
        st.what = "hipMemsetAsync";
        st.e = hipMemsetAsync(p, 0, sizeof(T) * count, s);
    }
};

struct DxMoments {
    int32_t sel[MAXC] = {};          // effective selection (bits as in include/dangx.h)
    int type[MAXC] = {}, nind[MAXC] = {};  // shape key recorded at begin
    struct Seg { int comp, what, plane; long long off; int id = 0; };   // id: its index in segs
    std::vector<Seg> segs;
    std::vector<MomSeg> table;       // the table as last uploaded
    DevBuf<MomSeg> d_table;
    DevBuf<double> acc;              // [mean: acc_half doubles | m2: acc_half doubles]
    long long acc_half = 0;
    long long count = 0;
    double tm_mean[MAXC][3][MAXB] = {}, tm_m2[MAXC][3][MAXB] = {};
    DevBuf<double> scratch;          // what the host form of a read-out copies from; grows on demand (ReadOut)
    size_t scratch_bytes = 0;
    unsigned grid_target = 0;        // blocks of a full-machine launch
    // dangx_moments_pairs
    bool lag1 = false;
    DevBuf<double> lag;              // [prev | first | P], acc_half doubles each, planes at the offsets of acc
    DevBuf<LagSeg> d_lag;
    struct Pair { int a, b; long long off; int id = 0; };   // indices into segs; off: the pair's plane in pc (at the phase of a's mean); id: its index in pairs
    std::vector<Pair> pairs;
    DevBuf<double> pc;
    DevBuf<PairSeg> d_pairs;
    double tm_prev[MAXC][3][MAXB] = {}, tm_first[MAXC][3][MAXB] = {}, tm_P[MAXC][3][MAXB] = {};
    // dangx_moments_hist
    // seg: index into segs; off: the records' first word in hrec; id: its index in hists.  kind: DX_HIST_RANGE_* (dx_hist_host.h);
    // a per-pixel registration keeps lo = -inf, hi = +inf (what declared it), its maps at roff in hrange once have_maps, and sum:
    // their checksum
    // a histogram of a registered signal: seg = -1 and sig = its index in sigs (else sig = -1)
    struct Hist { int seg; double lo, hi; long long off; int id = 0; int kind = 0; long long roff = 0; bool have_maps = false; uint64_t sum = 0; int sig = -1; };
    std::vector<Hist> hists;
    int hbins = 0, hbits = 0;
    DevBuf<uint32_t> hrec;           // every registration's records, each block at a multiple of 256 bytes
    DevBuf<HistSeg> d_hist;          // the global-range registrations, in registration order
    DevBuf<double> hrange;           // per-pixel registrations: [lo: hpitch doubles | hi: hpitch doubles] each, at the phase of the segment's accumulators
    long long hpitch = 0;            // doubles between lo and hi of a registration (live: npix rounded up to even; holder: npix, packed)
    DevBuf<HistPxSeg> d_histpx;      // the per-pixel registrations, in registration order
    int nhist_px = 0;                // how many registrations of state planes are per-pixel
    int nhist_sig = 0;               // how many registrations read a signal (filled by k_moments_signal<BP, true>, no launch of their own)
    // dangx_moments_signals
    struct Sig { int comp, band, kind; long long off; int id = 0; };   // off: the signal's mean plane in sacc; id: its index in sigs
    std::vector<Sig> sigs;
    std::vector<DxSigSeg> sig_plan;
    int sig_type[MAXC] = {}, sig_nind[MAXC] = {};   // shape key of the registered components at registration
    bool sig_used[MAXC] = {};
    std::vector<SigSeg> sig_table;   // the table as last uploaded
    DevBuf<SigSeg> d_sig;
    DevBuf<double> sacc;             // [mean: sacc_half doubles | m2: sacc_half doubles]
    long long sacc_half = 0;
    // dangx_moments_angles
    struct Ang { int comp, band; long long off; int id = 0; };   // off: the angle's Cbar plane in aacc; id: its index in angs
    std::vector<Ang> angs;
    std::vector<DxAngSeg> ang_plan;
    int ang_type[MAXC] = {}, ang_nind[MAXC] = {};   // shape key of the registered components at registration
    bool ang_used[MAXC] = {};
    std::vector<AngSeg> ang_table;   // the table as last uploaded
    DevBuf<AngSeg> d_ang;
    DevBuf<double> aacc;             // [Cbar: aacc_half doubles | Sbar: aacc_half doubles], every plane at the phase of the component's Q plane
    long long aacc_half = 0;
    // dangx_moments_fit
    struct Fit { int what, band, plane; long long off; int id = 0; };   // off: the item's mean plane in facc; id: its index in fits
    std::vector<Fit> fits;
    std::vector<DxFitSeg> fit_plan;
    std::vector<FitSeg> fit_table;   // the table as last uploaded
    DevBuf<FitSeg> d_fit;
    DevBuf<double> facc;             // [mean: facc_half doubles | m2: facc_half doubles]; k_moments_fit goes pixel by pixel: no phase to keep
    long long facc_half = 0;
    // dangx_moments_batches: [reg][batch][mean | m2][bpitch] in bacc, every plane at the 16-byte phase of its segment's main
    // accumulator (bpitch is even, so a registration's planes share the phase of its first)
    struct Batch { int seg; long long off; int id = 0; };   // seg: index into segs; off: batch 0's mean plane in bacc; id: its index in batches
    std::vector<Batch> batches;
    int nbatch = 0;
    long long batch_len = 0;         // the current L
    long long bpitch = 0;            // doubles between two planes of a registration
    DevBuf<double> bacc;
    DevBuf<MomSeg> d_batch;          // [nbatch][nreg]: row b is the table of a launch into batch b (uploaded with the main table)
    // dangx_chains_*: orders this chain's stream against the stream of the chain set's first context (created on first use)
    hipEvent_t chain_ev = nullptr;

    DxMoments() = default;
    DxMoments(const DxMoments&) = delete;
    DxMoments& operator=(const DxMoments&) = delete;
    ~DxMoments() { if (chain_ev) (void)hipEventDestroy(chain_ev); }

    // dangx_moments_begin_like: a HOLDER has the registrations of another context and none of the allocations above.  Every section
    // (dx_section_host.h) put into it lives in a buffer of its own, allocated at its first put and packed as the section's payload
    // is; the tables below say where each plane of it lies (null: that section was not put).  Batches keep the pitch bpitch of a
    // live context, which the kernels over several chains take from chain 0.
    bool holder = false;
    bool head_put = false;            // a holder's count and batch bookkeeping were put
    struct Held { int family, a, b; DevBuf<unsigned char> buf; size_t bytes; };   // bytes: as allocated (a multiple of 256)
    std::vector<Held> held;
    struct HeldSeg { double *mean = nullptr, *m2 = nullptr, *prev = nullptr, *first = nullptr, *P = nullptr; };
    std::vector<HeldSeg> h_seg;       // by Seg::id
    std::vector<double*> h_pair;      // by Pair::id
    std::vector<uint32_t*> h_hist;    // by Hist::id
    std::vector<double*> h_range;     // by Hist::id: lo of a HIST_RANGE section put (hi follows at npix)
    std::vector<HeldSeg> h_sig;       // by Sig::id (mean, m2)
    std::vector<double*> h_batch;     // by Batch::id: batch 0's mean plane
    std::vector<HeldSeg> h_ang;       // by Ang::id (mean: Cbar, m2: Sbar)
    std::vector<HeldSeg> h_fit;       // by Fit::id (mean, m2)
    bool h_rows[MAXC] = {};           // the host rows tm_* of a template / monopole / hi_fit member were put

    // where things are
    double* mean(const Seg& s) const { return holder ? h_seg[s.id].mean : acc + s.off; }
    double* m2(const Seg& s) const { return holder ? h_seg[s.id].m2 : acc + acc_half + s.off; }
    double* prev(const Seg& s) const { return holder ? h_seg[s.id].prev : lag + s.off; }
    double* first(const Seg& s) const { return holder ? h_seg[s.id].first : lag + acc_half + s.off; }
    double* P(const Seg& s) const { return holder ? h_seg[s.id].P : lag + 2 * acc_half + s.off; }
    double* C(const Pair& p) const { return holder ? h_pair[p.id] : pc + p.off; }
    double* mean(const Sig& s) const { return holder ? h_sig[s.id].mean : sacc + s.off; }
    double* m2(const Sig& s) const { return holder ? h_sig[s.id].m2 : sacc + sacc_half + s.off; }
    double* angC(const Ang& a) const { return holder ? h_ang[a.id].mean : aacc + a.off; }
    double* angS(const Ang& a) const { return holder ? h_ang[a.id].m2 : aacc + aacc_half + a.off; }
    double* mean(const Fit& f) const { return holder ? h_fit[f.id].mean : facc + f.off; }
    double* m2(const Fit& f) const { return holder ? h_fit[f.id].m2 : facc + facc_half + f.off; }
    uint32_t* records(const Hist& h) const { return holder ? h_hist[h.id] : hrec + h.off; }
    double* range_lo(const Hist& h) const { return holder ? h_range[h.id] : (h.have_maps ? hrange + h.roff : nullptr); }   // null: no maps (yet)
    double* range_hi(const Hist& h) const { double* p = range_lo(h); return p ? p + hpitch : nullptr; }
    double* bbase(const Batch& r) const { return holder ? h_batch[r.id] : bacc + r.off; }
    double* bmean(const Batch& r, int b) const { double* p = bbase(r); return p ? p + 2LL * b * bpitch : nullptr; }
    double* bm2(const Batch& r, int b) const { double* p = bbase(r); return p ? p + (2LL * b + 1) * bpitch : nullptr; }
    int find_seg(int comp, int what, int plane) const {   // index into segs, -1: not selected
        for (size_t i = 0; i < segs.size(); ++i)
            if (segs[i].comp == comp && segs[i].what == what && segs[i].plane == plane) return (int)i;
        return -1;
    }
    // blocks per row of a launch of `rows` rows (blockIdx.y) over `items` items each: together about one full machine
    unsigned grid_for(long long items, unsigned rows) const { return std::max(1u, std::min(nblocks(items), (grid_target + rows - 1) / rows)); }
};

inline bool same_plane(const DxMoments::Seg& x, const DxMoments::Seg& y) { return x.comp == y.comp && x.what == y.what && x.plane == y.plane; }

// A read-out's destination.  Device form: the caller's buffer, and close() does nothing.  Host form: the context's scratch buffer
// (grown here to `bytes` when it is smaller, after a wait for whatever still reads the old one), which close() copies to the
// caller's array and waits for.
struct ReadOut {
    dangx_ctx* ctx;
    double* out;
    bool to_host;
    double* dst = nullptr;   // where the kernel writes: valid after open()
    int open(size_t bytes) {
        dst = out;
        if (!to_host) return 0;
        DxMoments* m = ctx->mom;
        if (bytes > m->scratch_bytes) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            m->scratch = DevBuf<double>();
            m->scratch_bytes = 0;
            HIPCHK(ctx, hipMalloc(&m->scratch.p, bytes));
            m->scratch_bytes = bytes;
        }
        dst = m->scratch;
        return 0;
    }
    // the planes named by `planes` (bit k) of dst's [nplanes][n], host_stride doubles apart in the caller's array
    int close(unsigned planes, int nplanes, long long n, long long host_stride) {
        if (!to_host) return 0;
        for (int k = 0; k < nplanes; ++k)
            if ((planes >> k) & 1u)
                HIPCHK(ctx, hipMemcpyAsync(out + (long long)k * host_stride, dst + (long long)k * n, sizeof(double) * (size_t)n,
                                           hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    }
    int close(long long n) { return close(1u, 1, n, n); }   // one run of n doubles
};

// "no sample accumulated", and for a stat that divides by n - ddof (noun names it in the message) the range of ddof
inline int count_check(dangx_ctx* ctx, const char* noun, int ddof) {
    const long long n = ctx->mom->count;
    if (n == 0) return fail(ctx, "posterior moments: no sample accumulated");
    if (noun && (ddof < 0 || n - ddof <= 0)) return fail(ctx, std::string("posterior moments: ") + noun + " needs 0 <= ddof < n");
    return 0;
}

int dx_hist_stat_check(dangx_ctx* ctx, int reg, int stat, int nq, const double* q);   // dangx_moments.hip: the checks of a histogram read-out
