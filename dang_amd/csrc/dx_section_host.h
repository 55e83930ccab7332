// dx_section_host.h -- the sections of a context's accumulator state (dangx_moments_section_*, include/dangx.h): their packed
// payloads, the HEAD record and the fingerprint of a registration.  Pure host code without the HIP runtime: dangx_moments.hip
// and a stand-alone host program use the same functions.
//
// A section is addressed by (family, a, b); its payload is packed, little-endian and independent of where the context keeps it:
//   HEAD    (-, -)        DX_SEC_HEAD_BYTES bytes, host only (DxSecHead below)
//   PLANES  (comp, what)  parts mean, m2 (then prev, first, P when lag-1 is tracked), each [selected planes in T, Q, U order][npix]
//                         f64; for a template / monopole / hi_fit member (what 0) the host rows, each [selected planes][nbands]
//   PAIR    (pair, -)     C[npix] f64
//   HIST    (reg, -)      [npix][nbins] counters of `bits` bits, as dangx_moments_hist_get lays them out
//   SIGNAL  (sig, -)      mean, m2, each [npix] f64
//   BATCHES (reg, -)      [nbatch][mean, m2][npix] f64
//   HIST_RANGE (reg, -)   lo, hi, each [npix] f64: the range maps of a histogram registration with per-pixel ranges (only those have it)
//   ANGLE   (ang, -)      Cbar, Sbar, each [npix] f64 (dx_angle_host.h)
//   FIT     (item, -)     mean, m2, each [npix] f64 (dx_fit_host.h): family DX_SEC_FIT = 8, which exists only in a context with fit
//                         items -- DX_SEC_FAMILIES counts the families every context has
//
// The fingerprint is FNV-1a (64 bit) over the registration written out as little-endian 64-bit words, in six groups that HEAD
// carries one by one, so that a mismatch can be named: the shard (npix, pix0, nmaps), the selection (the selection words, type
// and nindices of every selected component), the pairs (lag-1 flag and pair list), the histograms (planes, lo, hi as their bit
// patterns, nbins, bits; with a per-pixel range anywhere in the list also every registration's range kind and the checksum of its
// maps -- a list of global ranges alone hashes as it always did), the signals (specs; with an angle registered also the angle
// specs, and with a fit item registered the fit specs -- a registration without angles / fit items hashes as it always did) and the batches (planes, nbatch).  The overall value hashes
// the six.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

enum { DX_SEC_HEAD = 0, DX_SEC_PLANES = 1, DX_SEC_PAIR = 2, DX_SEC_HIST = 3, DX_SEC_SIGNAL = 4, DX_SEC_BATCHES = 5, DX_SEC_HIST_RANGE = 6, DX_SEC_ANGLE = 7, DX_SEC_FAMILIES = 8 };
enum { DX_SEC_FIT = 8 };   // behind the families every context has
enum { DX_SEC_G_SHARD = 0, DX_SEC_G_SEL = 1, DX_SEC_G_PAIRS = 2, DX_SEC_G_HIST = 3, DX_SEC_G_SIGNALS = 4, DX_SEC_G_BATCHES = 5, DX_SEC_GROUPS = 6 };

#define DX_SEC_VERSION 1u
#define DX_SEC_MAGIC 0x48535844u   // "DXSH" read as a little-endian word
#define DX_SEC_HEAD_BYTES 104

inline const char* dx_section_family_name(int family) {
    static const char* const n[DX_SEC_FAMILIES] = {"HEAD", "PLANES", "PAIR", "HIST", "SIGNAL", "BATCHES", "HIST_RANGE", "ANGLE"};
    if (family == DX_SEC_FIT) return "FIT";
    return family >= 0 && family < DX_SEC_FAMILIES ? n[family] : "?";
}

struct DxSecReg {              // what a registration is made of
    long long npix = 0, pix0 = 0;
    int nmaps = 0;
    std::vector<int32_t> sel, type, nind;     // per component; type and nind count where sel != 0 only
    int lag1 = 0;
    std::vector<int32_t> pairs;               // 6 per pair: {comp, what, plane} of a and of b
    std::vector<int32_t> hist_planes;         // 3 per registration
    std::vector<double> hist_range;           // lo, hi per registration ({-inf, +inf}: per-pixel maps)
    std::vector<int32_t> hist_kind;           // range kind per registration (dx_hist_host.h); empty or all 0: global ranges only
    std::vector<uint64_t> hist_sum;           // checksum of the range maps per registration (0 for a global range)
    int nbins = 0, bits = 0;
    std::vector<int32_t> signals;             // 3 per signal: {comp, band, kind}
    std::vector<int32_t> angles;              // 2 per angle: {comp, band}; hashed into the signals' group, and only when not empty
    std::vector<int32_t> fit;                 // 3 per fit item: {what, band, plane}; hashed into the signals' group behind a marker word, and only when not empty
    std::vector<int32_t> batch_planes;        // 3 per registration
    int nbatch = 0;
};

struct DxSecHead {
    uint32_t magic = DX_SEC_MAGIC, version = DX_SEC_VERSION;
    int64_t count = 0;
    int32_t lag1 = 0, nbatch = 0;
    int64_t batch_len = 0;                    // 0 without batches
    int32_t nfull = 0, reserved = 0;          // full batches
    int64_t partial = 0;                      // samples in the open batch
    uint64_t fingerprint = 0;
    uint64_t group[DX_SEC_GROUPS] = {};
};

struct DxSecHash {
    uint64_t h = 0xcbf29ce484222325ull;
    void word(uint64_t v) {
        for (int i = 0; i < 8; ++i) {
            h ^= (v >> (8 * i)) & 0xffu;
            h *= 0x100000001b3ull;
        }
    }
    void num(long long v) { word((uint64_t)v); }
    void real(double v) {
        uint64_t u;
        std::memcpy(&u, &v, sizeof u);
        word(u);
    }
    void list(const std::vector<int32_t>& v) {
        num((long long)v.size());
        for (int32_t x : v) num(x);
    }
};

inline void dx_section_groups(const DxSecReg& r, uint64_t (&g)[DX_SEC_GROUPS]) {
    DxSecHash a, b, c, d, e, f;
    a.num(r.npix); a.num(r.pix0); a.num(r.nmaps);
    b.list(r.sel);
    for (size_t l = 0; l < r.sel.size(); ++l) {
        const bool on = r.sel[l] != 0;
        b.num(on && l < r.type.size() ? r.type[l] : 0);
        b.num(on && l < r.nind.size() ? r.nind[l] : 0);
    }
    c.num(r.lag1 ? 1 : 0); c.list(r.pairs);
    d.list(r.hist_planes);
    d.num((long long)r.hist_range.size());
    for (double v : r.hist_range) d.real(v);
    d.num(r.hist_planes.empty() ? 0 : r.nbins); d.num(r.hist_planes.empty() ? 0 : r.bits);
    bool per_pixel = false;
    for (int32_t k : r.hist_kind) per_pixel = per_pixel || k != 0;
    if (per_pixel) {   // only then: the group of a list of global ranges stays what it was
        d.list(r.hist_kind);
        d.num((long long)r.hist_sum.size());
        for (uint64_t v : r.hist_sum) d.word(v);
    }
    e.list(r.signals);
    if (!r.angles.empty()) e.list(r.angles);   // only then: the group of a registration without angles stays what it was
    if (!r.fit.empty()) {                      // likewise; the marker keeps a fit list apart from an angle list of the same numbers
        e.word(0x544946ull);                   // "FIT"
        e.list(r.fit);
    }
    f.list(r.batch_planes); f.num(r.batch_planes.empty() ? 0 : r.nbatch);
    g[0] = a.h; g[1] = b.h; g[2] = c.h; g[3] = d.h; g[4] = e.h; g[5] = f.h;
}

inline uint64_t dx_section_fingerprint(const uint64_t (&g)[DX_SEC_GROUPS]) {
    DxSecHash t;
    for (int i = 0; i < DX_SEC_GROUPS; ++i) t.word(g[i]);
    return t.h;
}

inline uint64_t dx_section_fingerprint(const DxSecReg& r) {
    uint64_t g[DX_SEC_GROUPS];
    dx_section_groups(r, g);
    return dx_section_fingerprint(g);
}

// the HEAD of a context with this registration and this much accumulated
inline DxSecHead dx_section_head(const DxSecReg& r, long long count, long long batch_len) {
    DxSecHead h;
    h.count = count;
    h.lag1 = r.lag1 ? 1 : 0;
    const bool batched = !r.batch_planes.empty();
    h.nbatch = batched ? r.nbatch : 0;
    h.batch_len = batched ? batch_len : 0;
    h.nfull = batched && batch_len > 0 ? (int32_t)(count / batch_len) : 0;
    h.partial = batched && batch_len > 0 ? count % batch_len : 0;
    dx_section_groups(r, h.group);
    h.fingerprint = dx_section_fingerprint(h.group);
    return h;
}

inline void dx_sec_put32(unsigned char*& p, uint32_t v) { for (int i = 0; i < 4; ++i) *p++ = (unsigned char)(v >> (8 * i)); }
inline void dx_sec_put64(unsigned char*& p, uint64_t v) { for (int i = 0; i < 8; ++i) *p++ = (unsigned char)(v >> (8 * i)); }
inline uint32_t dx_sec_get32(const unsigned char*& p) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)*p++ << (8 * i); return v; }
inline uint64_t dx_sec_get64(const unsigned char*& p) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= (uint64_t)*p++ << (8 * i); return v; }

inline void dx_section_head_pack(const DxSecHead& h, unsigned char* out) {   // out: DX_SEC_HEAD_BYTES
    unsigned char* p = out;
    dx_sec_put32(p, h.magic); dx_sec_put32(p, h.version);
    dx_sec_put64(p, (uint64_t)h.count);
    dx_sec_put32(p, (uint32_t)h.lag1); dx_sec_put32(p, (uint32_t)h.nbatch);
    dx_sec_put64(p, (uint64_t)h.batch_len);
    dx_sec_put32(p, (uint32_t)h.nfull); dx_sec_put32(p, (uint32_t)h.reserved);
    dx_sec_put64(p, (uint64_t)h.partial);
    dx_sec_put64(p, h.fingerprint);
    for (int i = 0; i < DX_SEC_GROUPS; ++i) dx_sec_put64(p, h.group[i]);
}

// "" or why the bytes are no HEAD of this version: truncated, foreign, or fields that contradict one another
inline std::string dx_section_head_unpack(const unsigned char* in, size_t bytes, DxSecHead& h) {
    if (!in || bytes != DX_SEC_HEAD_BYTES)
        return "a HEAD section is " + std::to_string(DX_SEC_HEAD_BYTES) + " bytes, not " + std::to_string(bytes) + " (truncated or foreign)";
    const unsigned char* p = in;
    h.magic = dx_sec_get32(p); h.version = dx_sec_get32(p);
    h.count = (int64_t)dx_sec_get64(p);
    h.lag1 = (int32_t)dx_sec_get32(p); h.nbatch = (int32_t)dx_sec_get32(p);
    h.batch_len = (int64_t)dx_sec_get64(p);
    h.nfull = (int32_t)dx_sec_get32(p); h.reserved = (int32_t)dx_sec_get32(p);
    h.partial = (int64_t)dx_sec_get64(p);
    h.fingerprint = dx_sec_get64(p);
    for (int i = 0; i < DX_SEC_GROUPS; ++i) h.group[i] = dx_sec_get64(p);
    if (h.magic != DX_SEC_MAGIC) return "not a HEAD section (foreign bytes: the magic word is missing)";
    if (h.version != DX_SEC_VERSION) return "HEAD has layout version " + std::to_string(h.version) + ", this library reads version " + std::to_string(DX_SEC_VERSION);
    if (h.fingerprint != dx_section_fingerprint(h.group)) return "HEAD is damaged (its fingerprint is not that of its groups)";
    if (h.count < 0 || (h.lag1 != 0 && h.lag1 != 1) || h.nbatch < 0) return "HEAD is damaged (a negative count or nbatch, or a lag-1 flag that is not 0 or 1)";
    if (h.nbatch == 0) {
        if (h.batch_len != 0 || h.nfull != 0 || h.partial != 0) return "HEAD is damaged (batch bookkeeping without batches)";
    } else {
        if (h.batch_len < 1) return "HEAD is damaged (batch_len < 1)";
        if (h.nfull != h.count / h.batch_len || h.partial != h.count % h.batch_len || h.nfull > h.nbatch)
            return "HEAD is damaged (count, batch_len, the full batches and the fill of the open batch contradict one another)";
    }
    return "";
}

// "" when `got` describes the registration of `own`, else what differs
inline std::string dx_section_head_diff(const DxSecHead& got, const DxSecHead& own) {
    static const char* const what[DX_SEC_GROUPS] = {
        "the shard (npix, pix0 or nmaps)", "the selection (selection words, type or nindices of a selected component)",
        "the pair list", "the histogram registrations (planes, lo / hi range, nbins or bits)", "the fit items, signal or angle registrations",
        "the batch registrations (planes)"};
    std::string why;
    auto add = [&](const std::string& s) { why += (why.empty() ? "" : "; ") + s; };
    if (got.lag1 != own.lag1) add(got.lag1 ? "lag-1 is tracked there and missing here" : "lag-1 is missing there and tracked here");
    if (got.nbatch != own.nbatch) add("nbatch is " + std::to_string(got.nbatch) + " there and " + std::to_string(own.nbatch) + " here");
    for (int i = 0; i < DX_SEC_GROUPS; ++i) {
        if (got.group[i] == own.group[i]) continue;
        if (i == DX_SEC_G_PAIRS && got.lag1 != own.lag1) {   // the flag is part of the group: named above, the list may agree
            continue;
        }
        if (i == DX_SEC_G_BATCHES && got.nbatch != own.nbatch) continue;
        add(std::string(what[i]) + " differ");
    }
    if (why.empty() && got.fingerprint != own.fingerprint) add("the fingerprints differ");
    return why;
}

// payload bytes.  n: npix (nbands for the host rows of a template / monopole / hi_fit member); nsel: selected planes of (comp, what)
inline long long dx_section_planes_parts(int lag1) { return lag1 ? 5 : 2; }
inline long long dx_section_planes_bytes(long long n, int nsel, int lag1) { return dx_section_planes_parts(lag1) * nsel * n * 8; }
inline long long dx_section_pair_bytes(long long npix) { return npix * 8; }
inline long long dx_section_hist_bytes(long long npix, int nbins, int bits) { return npix * nbins * (bits / 8); }
inline long long dx_section_signal_bytes(long long npix) { return 2 * npix * 8; }
inline long long dx_section_batches_bytes(long long npix, int nbatch) { return 2LL * nbatch * npix * 8; }
inline long long dx_section_hist_range_bytes(long long npix) { return 2 * npix * 8; }
inline long long dx_section_angle_bytes(long long npix) { return 2 * npix * 8; }
inline long long dx_section_fit_bytes(long long npix) { return 2 * npix * 8; }
inline long long dx_section_round256(long long bytes) { return (bytes + 255) / 256 * 256; }
