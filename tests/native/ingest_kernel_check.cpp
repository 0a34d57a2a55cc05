// TEST INFRASTRUCTURE: the kernels behind the device DEFLATE decoder -- all of mitoflex_amd/csrc/mf_ingest.hip and the de-duplication set of
// mf_kernels.hip -- called through their launch_* functions as the product calls them and held to plain host loops, one JSON line per case.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I mitoflex_amd/csrc -x hip ingest_kernel_check.cpp -x none build/mf_ingest.o build/mf_kernels.o
//     (mf_kernels.o links on its own: it needs nothing of the other objects, so the shared library is not used)
//   g++ -DINGEST_KERNEL_CHECK_STUB -I tests/native/hipstub -I mitoflex_amd/csrc ingest_kernel_check.cpp ingest_stub.cpp hipstub.cpp mf_pinflate.cpp ...
//     (the same cases against the stand-in loops of ingest_stub.cpp on the CPU: two independent plain implementations that must agree.  The
//     stand-in's hash is FNV, so under this switch the hash comparison is left out and the caller checks the printed reference values)
//   ingest_kernel_check scan | lines | seqlens | pack | select | qual | hash | decide | dedup | bytes
// Every reference here is a byte-at-a-time or element-at-a-time loop, written from the strings the text was made of wherever that is possible,
// and shares no helper with mf_ingest.hip.  All comparisons are exact.  Every buffer a kernel writes is larger than the right answer needs
// (SLACK entries) and lies between two canary zones (CAN entries), all preset to a pattern: a wrong kernel fails a comparison or `canary_wrong`
// instead of faulting.  Text has 64 readable bytes in front and behind, filled with LF and 'N' (a kernel that looks past n counts wrong), and
// is run with its first byte at every offset 0..15 from an aligned allocation (the product's text pointers are unaligned).
// QF_LONG needs a record of 4 GiB and is left out.
// Every HIP call is checked: the first error ends the run with exit status 2.  Results are for the caller to judge (the JSON fields).
#include "mf_ingest.h"
#include "mf_kernels.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <map>
#include <math.h>
#include <random>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace mf;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

#ifdef INGEST_KERNEL_CHECK_STUB
// (ingest_stub.cpp's stand-ins for mf_api.cpp allocate through mf_api_internal.h, which turns to the text-buffer pool of mf_devingest.cpp when
// the device is full; nothing here comes that way, and this spares the link all of the ingest path)
namespace mf { size_t release_cached_device_memory(bool) { return 0; } }
#endif

static hipStream_t g_st;
static void sync_st() { CK(hipStreamSynchronize(g_st)); }

constexpr size_t CAN = 64, SLACK = 16;
constexpr uint8_t PAT = 0xA5;
static uint64_t g_canary;          // bytes outside the expected answer that lost the pattern, of the case being run

// a device array: n entries for the answer, SLACK more, CAN in front and behind, every byte PAT
template <class T> struct Dev {
    T *raw = nullptr; size_t n;
    explicit Dev(size_t n_) : n(n_)
    {
        const size_t tot = n + SLACK + 2 * CAN;
        CK(hipMalloc(&raw, tot * sizeof(T)));
        std::vector<uint8_t> f(tot * sizeof(T), PAT);
        CK(hipMemcpy(raw, f.data(), f.size(), hipMemcpyHostToDevice));
    }
    Dev(const Dev &) = delete;
    ~Dev() { CK(hipFree(raw)); }
    T *p() const { return raw + CAN; }
    void put(const std::vector<T> &v, size_t at = 0) { if (!v.empty()) CK(hipMemcpy(p() + at, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); }
    // the first `want` entries; every byte behind them and in the canary zones must still hold the pattern
    std::vector<T> get(size_t want)
    {
        const size_t tot = n + SLACK + 2 * CAN;
        if (want > n + SLACK) { fprintf(stderr, "driver: get(%zu) of %zu\n", want, n); exit(3); }
        std::vector<T> all(tot);
        CK(hipMemcpy(all.data(), raw, tot * sizeof(T), hipMemcpyDeviceToHost));
        const uint8_t *b = reinterpret_cast<const uint8_t *>(all.data());
        for (size_t i = 0; i < tot * sizeof(T); i++) if ((i < CAN * sizeof(T) || i >= (CAN + want) * sizeof(T)) && b[i] != PAT) g_canary++;
        return std::vector<T>(all.begin() + CAN, all.begin() + CAN + want);
    }
};

// text on the device, its first byte `off` bytes behind a 16-aligned address
struct Text {
    uint8_t *raw = nullptr, *p = nullptr;
    Text(const std::vector<uint8_t> &t, unsigned off)
    {
        std::vector<uint8_t> h(64 + 16 + t.size() + 64);
        for (size_t i = 0; i < h.size(); i++) h[i] = (i & 1) ? 'N' : '\n';
        if (!t.empty()) memcpy(h.data() + 64 + off, t.data(), t.size());
        CK(hipMalloc(&raw, h.size()));
        CK(hipMemcpy(raw, h.data(), h.size(), hipMemcpyHostToDevice));
        p = raw + 64 + off;
    }
    Text(const Text &) = delete;
    ~Text() { CK(hipFree(raw)); }
};

struct J {
    std::string s;
    explicit J(const char *mode) { s = std::string("{\"mode\":\"") + mode + "\""; g_canary = 0; }
    J &u(const char *k, uint64_t v) { char b[96]; snprintf(b, sizeof b, ",\"%s\":%llu", k, (unsigned long long)v); s += b; return *this; }
    J &str(const char *k, const std::string &v) { s += std::string(",\"") + k + "\":\"" + v + "\""; return *this; }
    J &raw(const char *k, const std::string &v) { s += std::string(",\"") + k + "\":" + v; return *this; }
    void emit() { u("canary_wrong", g_canary); s += "}"; puts(s.c_str()); fflush(stdout); }
};

template <class T> static uint64_t diff(const std::vector<T> &a, const std::vector<T> &b)
{
    uint64_t d = a.size() > b.size() ? a.size() - b.size() : b.size() - a.size();
    for (size_t i = 0; i < std::min(a.size(), b.size()); i++) d += a[i] != b[i];
    return d;
}

static std::vector<uint64_t> ref_scan(const std::vector<uint32_t> &in)
{
    std::vector<uint64_t> o(in.size() + 1); uint64_t s = 0;
    for (size_t i = 0; i < in.size(); i++) { o[i] = s; s += in[i]; }
    o[in.size()] = s;
    return o;
}
// the device's scan of `in` (the product's launch_scan_u32), n + 1 values
static std::vector<uint64_t> dev_scan(const std::vector<uint32_t> &in, Dev<uint64_t> &d_out)
{
    const uint64_t n = in.size();
    Dev<uint32_t> d_in(n); d_in.put(in);
    Dev<uint64_t> d_scr(n / 4096 + 2);
    CK(launch_scan_u32(d_in.p(), n, d_out.p(), d_scr.p(), g_st)); sync_st();
    (void)d_scr.get(n / 4096 + 2);
    return d_out.get(n + 1);
}

// ------------------------------------------------------------------------------------------------------------------------------ FASTQ text
struct Spec { std::string h, s, plus = "+", q; };
struct Fastq {
    std::vector<uint8_t> text; std::vector<uint64_t> ls;       // ls: the line index as index_piece leaves it (an open last line ends at a virtual n + 1)
    std::vector<Spec> eff;                                     // the lines as the readers see them: without a CR in front of the LF
};
static std::string seen_line(const std::string &l, bool crlf) { return !crlf && !l.empty() && l.back() == '\r' ? l.substr(0, l.size() - 1) : l; }
static Fastq make_fastq(const std::vector<Spec> &recs, bool crlf, bool open_end)
{
    Fastq f; std::string t; const std::string eol = crlf ? "\r\n" : "\n";
    for (const Spec &r : recs) { t += r.h + eol + r.s + eol + r.plus + eol + r.q + eol; f.eff.push_back(Spec{seen_line(r.h, crlf), seen_line(r.s, crlf), r.plus, seen_line(r.q, crlf)}); }
    if (open_end) { if (recs.empty() || recs.back().q.empty()) { fprintf(stderr, "driver: open end needs a last quality line\n"); exit(3); } t.resize(t.size() - eol.size()); }
    f.text.assign(t.begin(), t.end());
    f.ls.push_back(0);
    for (size_t i = 0; i < t.size(); i++) if (t[i] == '\n') f.ls.push_back(i + 1);
    if (!t.empty() && t.back() != '\n') f.ls.push_back(t.size() + 1);
    if (f.ls.size() != 4 * recs.size() + 1) { fprintf(stderr, "driver: a line of the text holds an LF\n"); exit(3); }
    return f;
}
static std::string rnd_str(std::mt19937_64 &g, size_t n, const char *alphabet)
{
    const size_t k = strlen(alphabet); std::string s(n, ' ');
    for (size_t i = 0; i < n; i++) s[i] = alphabet[g() % k];
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------ scan
static void mode_scan()
{
    const uint64_t P = 256ull * 4096, sizes[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, P - 1, P, P + 1, 3 * P + 5};
    const char *kinds[] = {"zero", "one", "max", "random"};
    std::mt19937_64 g(1);
    for (uint64_t n : sizes) for (int kind = 0; kind < 4; kind++) {
        std::vector<uint32_t> in(n);
        for (auto &v : in) v = kind == 0 ? 0u : kind == 1 ? 1u : kind == 2 ? 0xFFFFFFFFu : (uint32_t)g();
        J j("scan");
        Dev<uint64_t> d_out(n + 1);
        const auto out = dev_scan(in, d_out);
        j.u("n", n).str("values", kinds[kind]).u("partials", (n + 4095) / 4096).u("wrong", diff(out, ref_scan(in))).emit();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ lines
static void mode_lines()
{
    const uint64_t sizes[] = {1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5, 1000003};
    const char *pats[] = {"none", "all", "tile_edges", "lane_edges", "random_closed", "random_open"};
    std::mt19937_64 g(2);
    for (uint64_t n : sizes) for (int pat = 0; pat < 6; pat++) {
        std::vector<uint8_t> t(n);
        for (uint64_t i = 0; i < n; i++) {
            bool nl = false;
            switch (pat) {
            case 1: nl = true; break;
            case 2: nl = i % 4096 == 4095 || i % 4096 == 0; break;          // the last byte of every tile and the first
            case 3: nl = i % 32 == 15 || i % 32 == 16; break;               // the last byte of a lane's sixteen and the first of the next lane's
            case 4: case 5: nl = g() % 40 == 0; break;
            }
            t[i] = nl ? '\n' : "ACGTN@+I"[g() % 8];
        }
        if (pat == 4) t[n - 1] = '\n';
        if (pat == 5 || pat == 0) t[n - 1] = 'A';
        const uint64_t tiles = (n + INGEST_TILE - 1) / INGEST_TILE;
        std::vector<uint32_t> cnt(tiles, 0); std::vector<uint64_t> ls{0};
        for (uint64_t i = 0; i < n; i++) if (t[i] == '\n') { cnt[i / INGEST_TILE]++; ls.push_back(i + 1); }
        J j("lines");
        uint64_t cnt_wrong = 0, ls_wrong = 0;
        for (unsigned off = 0; off < 16; off++) {
            Text tx(t, off);
            Dev<uint32_t> d_cnt(tiles);
            CK(launch_count_newlines(tx.p, n, d_cnt.p(), g_st)); sync_st();
            const auto c = d_cnt.get(tiles);
            cnt_wrong += diff(c, cnt);
            Dev<uint64_t> d_base(tiles + 1);
            (void)dev_scan(cnt, d_base);                                    // (of the right counts: each kernel gets right inputs)
            Dev<uint64_t> d_ls(ls.size());
            CK(launch_line_starts(tx.p, n, d_base.p(), d_ls.p(), g_st)); sync_st();
            ls_wrong += diff(d_ls.get(ls.size()), ls);
        }
        j.u("n", n).str("pattern", pats[pat]).u("newlines", ls.size() - 1).u("ends_in_newline", t[n - 1] == '\n').u("offsets", 16)
            .u("tile_cnt_wrong", cnt_wrong).u("line_start_wrong", ls_wrong).emit();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ seqlens
static void mode_seqlens()
{
    const uint64_t sizes[] = {1, 63, 64, 65, 255, 256, 257, 1000};
    std::mt19937_64 g(3);
    for (uint64_t n_rec : sizes) for (int variant = 0; variant < 4; variant++) {          // LF, CRLF, LF open end, CRLF open end
        const bool crlf = variant & 1, open_end = variant >= 2;
        std::vector<Spec> recs(n_rec);
        for (uint64_t r = 0; r < n_rec; r++) {
            const unsigned kind = (unsigned)(g() % 8);
            const size_t len = kind == 0 ? 0 : kind == 1 ? 1 : (size_t)(g() % 300);
            recs[r].h = "@" + rnd_str(g, g() % 20, "abc:/0123");
            recs[r].s = kind == 2 ? std::string("\r") : kind == 3 ? rnd_str(g, len, "ACGT") + "\r" : rnd_str(g, len, "ACGTN");          // a CR of its own in front of the line end
            recs[r].q = rnd_str(g, std::max<size_t>(len, 1), "I5#F");
        }
        const Fastq f = make_fastq(recs, crlf, open_end);
        std::vector<uint32_t> want(n_rec); uint32_t mn = ~0u, mx = 0; uint64_t empty = 0, cr_only = 0;
        for (uint64_t r = 0; r < n_rec; r++) { want[r] = (uint32_t)f.eff[r].s.size(); mn = std::min(mn, want[r]); mx = std::max(mx, want[r]); empty += recs[r].s.empty(); cr_only += recs[r].s == "\r"; }
        J j("seqlens");
        uint64_t len_wrong = 0, minmax_wrong = 0;
        for (unsigned off = 0; off < 16; off++) {
            Text tx(f.text, off);
            Dev<uint64_t> d_ls(f.ls.size()); d_ls.put(f.ls);
            Dev<uint32_t> d_len(n_rec), d_mm(2); d_mm.put({~0u, 0u});
            CK(launch_seq_lens(tx.p, d_ls.p(), n_rec, d_len.p(), d_mm.p(), g_st)); sync_st();
            len_wrong += diff(d_len.get(n_rec), want);
            minmax_wrong += diff(d_mm.get(2), std::vector<uint32_t>{mn, mx});
            (void)d_ls.get(f.ls.size());
        }
        j.u("n_rec", n_rec).u("crlf", crlf).u("open_end", open_end).u("empty_lines", empty).u("cr_only_lines", cr_only).u("offsets", 16)
            .u("seq_len_wrong", len_wrong).u("minmax_wrong", minmax_wrong).emit();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ pack
static int base_code(uint8_t c)
{
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; }
    return -1;
}
static std::string noisy_read(std::mt19937_64 &g, size_t len)
{
    static const char bad[] = {'@', '`', 'N', 'n', '.', '\r', (char)0x80, (char)0xFF, '[', 'U', '\0', ' '};
    std::string s(len, 'A');
    for (size_t i = 0; i < len; i++) s[i] = g() % 24 == 0 ? bad[g() % sizeof bad] : "ACGTacgt"[g() % 8];
    if (len && s.back() == '\r') s.back() = 'N';          // (a CR in front of the line end is no base)
    return s;
}
static void pack_case(const char *name, const std::vector<std::string> &reads, uint32_t uniform_len)
{
    const uint64_t bases[] = {0, 1, 15, 16, 17, 65533};
    std::vector<Spec> recs;
    for (const auto &s : reads) recs.push_back(Spec{"@r", s, "+", std::string(s.size(), 'I')});
    const Fastq f = make_fastq(recs, false, false);
    const uint64_t n_rec = reads.size();
    std::vector<uint64_t> offsets(n_rec + 1, 0); std::vector<uint8_t> stream; std::vector<uint32_t> rid;
    uint64_t empty_runs = 0;
    for (uint64_t r = 0; r < n_rec; r++) {
        offsets[r + 1] = offsets[r] + reads[r].size();
        for (char c : reads[r]) { stream.push_back((uint8_t)c); rid.push_back((uint32_t)r); }
        if (reads[r].empty() && (r == 0 || !reads[r - 1].empty())) empty_runs++;
    }
    const uint64_t total = stream.size();
    std::mt19937_64 g(4);
    for (uint64_t base : bases) {
        const uint64_t w0 = base >> 4, w_end = (base + total + 15) >> 4, pre_words = (base + 15) >> 4;
        std::vector<uint32_t> pre(pre_words);                       // the batches in front: their last word is complete, zero behind their last base
        for (auto &v : pre) v = (uint32_t)g() | 0x40000001u;
        if (base & 15) pre[pre_words - 1] = (pre[pre_words - 1] & ((1u << (2 * (base & 15))) - 1)) | 1u;
        std::vector<uint32_t> want_words(pre); want_words.resize(std::max(w_end, pre_words), 0);
        const uint64_t nb = total ? (w_end - w0 + 255) / 256 : 0;
        std::vector<uint32_t> want_cnt(nb, 0); std::vector<uint64_t> want_npos;
        uint64_t shared_invalid = 0, fast_words = 0, border_words = 0;
        for (uint64_t i = 0; i < total; i++) {
            const uint64_t gpos = base + i; const int c = base_code(stream[i]);
            if (c > 0) want_words[gpos >> 4] |= (uint32_t)c << (2 * (gpos & 15));
            if (c < 0) { want_cnt[((gpos >> 4) - w0) / 256]++; want_npos.push_back(gpos); if ((base & 15) && (gpos >> 4) == w0) shared_invalid++; }
        }
        for (uint64_t w = w0; w < w_end && total; w++) {            // which branch of the kernel each word of the batch is built to reach
            const uint64_t lo = std::max(w * 16, base), hi = std::min(w * 16 + 16, base + total);
            const uint32_t a = rid[lo - base], b = rid[hi - 1 - base];
            if (hi - lo == 16 && a == b) fast_words++;
            if (a != b) border_words++;
        }
        J j("pack");
        uint64_t words_wrong = 0, cnt_wrong = 0, npos_wrong = 0, blocks_wrong = pack_blocks(total, base) != nb;
        for (unsigned off = 0; off < 16 && !blocks_wrong; off++) {
            Text tx(f.text, off);
            Dev<uint64_t> d_ls(f.ls.size()), d_off(n_rec + 1); d_ls.put(f.ls); d_off.put(offsets);
            Dev<uint32_t> d_words(want_words.size()), d_cnt(nb); d_words.put(pre);
            const uint64_t *offp = uniform_len ? nullptr : d_off.p();
            CK(launch_pack(tx.p, d_ls.p(), offp, uniform_len, n_rec, total, base, d_words.p(), d_cnt.p(), nullptr, nullptr, g_st)); sync_st();
            words_wrong += diff(d_words.get(want_words.size()), want_words);
            const auto cnt = d_cnt.get(nb);
            cnt_wrong += diff(cnt, want_cnt);
            Dev<uint64_t> d_ib(nb + 1);
            const auto ib = dev_scan(cnt, d_ib);                     // (the device's own counts: mode 1 skips the workgroups whose count is 0)
            Dev<uint64_t> d_npos(std::max<uint64_t>(want_npos.size(), ib[nb]));          // room for what the device counted, right or wrong
            CK(launch_pack(tx.p, d_ls.p(), offp, uniform_len, n_rec, total, base, d_words.p(), d_cnt.p(), d_ib.p(), d_npos.p(), g_st)); sync_st();
            npos_wrong += diff(d_npos.get(want_npos.size()), want_npos);
            words_wrong += diff(d_words.get(want_words.size()), want_words);          // (mode 1 leaves the words alone)
        }
        j.str("case", name).u("uniform_len", uniform_len).u("n_rec", n_rec).u("total_bases", total).u("base", base).u("blocks", nb).u("invalid", want_npos.size())
            .u("shared_word_invalid", shared_invalid).u("fast_words", fast_words).u("border_words", border_words).u("empty_runs", empty_runs).u("offsets", 16)
            .u("blocks_wrong", blocks_wrong).u("words_wrong", words_wrong).u("inv_cnt_wrong", cnt_wrong).u("npos_wrong", npos_wrong).emit();
    }
}
static void mode_pack()
{
    std::mt19937_64 g(5);
    // every byte value but LF at every position mod 16 (255 = -1 mod 16: each round of the 255 values is shifted by one), then plain bases
    std::string big;
    for (int k = 0; k < 16; k++) for (int v = 0; v < 256; v++) if (v != '\n') big.push_back((char)v);
    big += rnd_str(g, 5000, "ACGTacgt");
    std::vector<std::string> ragged;
    for (size_t len : {0, 0, 0, 1, 15, 16, 17, 0, 0, 31, 150, 151, -1, 0, 16, 16, 16, 33, 5, 0, 0}) ragged.push_back(len == (size_t)-1 ? big : noisy_read(g, len));
    ragged[3] = "N";                                                 // the first base of the batch: an invalid one in the word shared with the batch in front
    pack_case("ragged_lengths", ragged, 0);
    std::vector<std::string> many;
    for (int i = 0; i < 300; i++) many.push_back(noisy_read(g, g() % 5 == 0 ? 0 : g() % 40));
    pack_case("ragged_many_short", many, 0);
    pack_case("ragged_all_empty", std::vector<std::string>(7, std::string()), 0);
    for (uint32_t len : {1u, 15u, 16u, 17u, 31u, 150u, 151u, 5000u}) {
        std::vector<std::string> u;
        for (int i = 0; i < (len == 5000 ? 3 : 37); i++) u.push_back(noisy_read(g, len));
        u[0][0] = '.';
        pack_case("uniform", u, len);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ select
static std::string rec_out(const Spec &e, const std::string &s, const std::string &q) { return e.h + "\n" + s + "\n+\n" + q + "\n"; }
static void mode_select()
{
    const size_t L[] = {0, 1, 63, 64, 65, 200};
    const char *vname[] = {"lf", "crlf", "plus_text", "lf_open_end", "crlf_open_end"};
    std::mt19937_64 g(6);
    std::vector<Spec> recs;
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) {
        Spec r; r.h = L[a] ? "@" + rnd_str(g, L[a] - 1, "abcXYZ:/_09") : ""; r.s = rnd_str(g, L[b], "ACGTN"); r.q = rnd_str(g, L[(a + b) % 6], "I5#F!~");
        recs.push_back(r);
    }
    recs.push_back(Spec{"@last", "ACGTA", "+", "IIII!"});
    const uint64_t n_rec = recs.size();
    struct List { const char *name; std::vector<uint32_t> sel; };
    std::vector<List> lists;
    lists.push_back({"one_first", {0}}); lists.push_back({"one_middle", {17}}); lists.push_back({"one_last", {(uint32_t)n_rec - 1}});
    { List l{"all", {}}; for (uint32_t i = 0; i < n_rec; i++) l.sel.push_back(i); lists.push_back(l); }
    { List l{"every_third", {}}; for (uint32_t i = 1; i < n_rec; i += 3) l.sel.push_back(i); lists.push_back(l); }
    for (uint32_t k : {3u, 4u, 5u}) { List l{"tail", {}}; for (uint32_t i = 0; i < k; i++) l.sel.push_back((uint32_t)n_rec - k + i); lists.push_back(l); }
    for (int variant = 0; variant < 5; variant++) {
        std::vector<Spec> rv = recs;
        if (variant == 2) for (auto &r : rv) r.plus = "+" + r.h;
        const Fastq f = make_fastq(rv, variant == 1 || variant == 4, variant >= 3);
        for (const List &l : lists) for (int pinned = 0; pinned < 2; pinned++) {
            const uint64_t n_sel = l.sel.size();
            std::vector<uint32_t> want_len; std::string want_out;
            for (uint32_t r : l.sel) { const std::string o = rec_out(f.eff[r], f.eff[r].s, f.eff[r].q); want_len.push_back((uint32_t)o.size()); want_out += o; }
            const std::vector<uint8_t> want_bytes(want_out.begin(), want_out.end());
            J j("select");
            uint64_t len_wrong = 0, out_wrong = 0;
            for (unsigned off = 0; off < 16; off++) {
                Text tx(f.text, off);
                Dev<uint64_t> d_ls(f.ls.size()); d_ls.put(f.ls);
                Dev<uint32_t> d_sel(n_sel); d_sel.put(l.sel);
                uint32_t *h_sel = nullptr;
                if (pinned) { CK(hipHostMalloc(&h_sel, n_sel * 4 + 64, hipHostMallocDefault)); memcpy(h_sel, l.sel.data(), n_sel * 4); }
                const uint32_t *sel = pinned ? h_sel : d_sel.p();
                Dev<uint32_t> d_len(n_sel);
                CK(launch_sel_lens(tx.p, d_ls.p(), sel, n_sel, d_len.p(), g_st)); sync_st();
                len_wrong += diff(d_len.get(n_sel), want_len);
                Dev<uint64_t> d_off(n_sel + 1);
                (void)dev_scan(want_len, d_off);
                Dev<uint8_t> d_out(want_bytes.size());
                CK(launch_sel_gather(tx.p, d_ls.p(), sel, n_sel, d_off.p(), d_out.p(), g_st)); sync_st();
                out_wrong += diff(d_out.get(want_bytes.size()), want_bytes);
                if (h_sel) CK(hipHostFree(h_sel));
            }
            j.str("text", vname[variant]).str("list", l.name).u("n_sel", n_sel).str("sel_memory", pinned ? "pinned" : "device").u("out_bytes", want_bytes.size()).u("offsets", 16)
                .u("out_len_wrong", len_wrong).u("out_wrong", out_wrong).emit();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ qual
struct QualWant { std::vector<uint32_t> bad, cut_sl, cut_ql, olen; std::vector<uint8_t> flags; uint32_t first_flag = ~0u; std::vector<std::string> s, q; };
static bool has_high(const std::string &l) { for (unsigned char c : l) if (c >= 0x80) return true; return false; }
static QualWant ref_qual(const Fastq &f, uint64_t start, uint64_t cap, uint32_t quality, uint64_t ns)
{
    QualWant w;
    for (size_t r = 0; r < f.eff.size(); r++) {
        const Spec &e = f.eff[r];
        uint32_t fl = 0;
        if (has_high(e.h) || has_high(e.s) || has_high(e.q)) fl |= QF_HIGH;           // (not the '+' line: nobody unwraps it)
        std::string cs, cq;
        if (start > e.s.size() || start > e.q.size()) fl |= QF_SHORT;                 // (no cut strings then: the reference panics)
        else { cs = e.s.substr(start, cap > e.s.size() ? std::string::npos : (size_t)cap); cq = e.q.substr(start, cap > e.q.size() ? std::string::npos : (size_t)cap); }
        uint64_t nn = 0; uint32_t nb = 0;
        for (unsigned char c : cs) nn += c == 'N';
        for (unsigned char c : cq) nb += c <= quality;
        if (nn > ns) fl |= QF_NFAIL;
        w.bad.push_back(nb); w.flags.push_back((uint8_t)fl); w.cut_sl.push_back((uint32_t)cs.size()); w.cut_ql.push_back((uint32_t)cq.size());
        w.olen.push_back((uint32_t)(e.h.size() + cs.size() + cq.size() + 5));
        if ((fl & (QF_HIGH | QF_SHORT)) && w.first_flag == ~0u) w.first_flag = (uint32_t)r;
        w.s.push_back(cs); w.q.push_back(cq);
    }
    return w;
}
static void mode_qual()
{
    const uint64_t starts[] = {0, 1, 5, 20000}, caps[] = {0, 1, 7, ~0ull}, nss[] = {0, 1, ~0ull};
    const uint32_t quals[] = {1, 33, 55, 100};
    int combo = 0;
    for (uint64_t start : starts) for (uint64_t cap : caps) for (uint32_t quality : quals) for (uint64_t ns : nss) {
        std::mt19937_64 g(700 + combo);
        const bool crlf = combo & 1; combo++;
        const char qok = (char)(quality + 1), qbad = (char)quality;
        std::vector<Spec> recs;
        uint64_t short_seq_only = 0, short_qual_only = 0;
        // every size of a record from the smallest up to 300 bytes (as LF text), then one of 10 kB: every tail of the 8 x 16-byte stride; header lengths
        // 1..16 put the cuts' borders at every byte phase
        for (uint32_t T = 6; T <= 301; T++) {
            const uint32_t k = T - 6;
            const uint32_t hl = T == 301 ? 9 : std::min<uint32_t>(1 + (k * 5) % 16, T - 5), rem = T == 301 ? 10001 : T - 5 - hl;
            const uint32_t sl = (k & 1) ? rem - rem / 2 : rem / 2, ql = rem - sl;
            Spec r; r.h = "@" + rnd_str(g, hl - 1, "abcXYZ:/_09");
            // the four places where a cut border can be off by one: the byte in front of the cut, its first, its last, the one behind
            const uint64_t at[4] = {start - 1, start, cap == ~0ull ? ~0ull : start + cap - 1, cap == ~0ull ? ~0ull : start + cap};
            r.s = rnd_str(g, sl, "ACGTn");
            if (k % 5 < 4) { if (at[k % 5] < sl) r.s[at[k % 5]] = 'N'; }
            else for (auto &c : r.s) if (g() % 16 == 0) c = 'N';
            r.q = std::string(ql, qok);
            switch (k % 7) {
            case 0: case 1: case 2: case 3: if (at[k % 7] < ql) r.q[at[k % 7]] = qbad; break;
            case 4: for (auto &c : r.q) { const char pick[] = {qbad, qok, 0x7F, '!', 1, 'I', '~'}; c = pick[g() % sizeof pick]; } break;
            case 5: for (auto &c : r.q) { const char pick[] = {qbad, qok, (char)0x80, (char)0xFF, (char)(0x80 | quality)}; c = pick[g() % sizeof pick]; } break;          // at or above 0x80: not "bad", and QF_HIGH
            case 6: r.q = std::string(ql, 0x7F); break;
            }
            short_seq_only += start > sl && start <= ql; short_qual_only += start > ql && start <= sl;
            recs.push_back(r);
        }
        if (start) {          // too short for the cut by one byte, from the sequence alone and from the quality string alone
            recs.push_back(Spec{"@short_seq", rnd_str(g, start - 1, "ACGTN"), "+", std::string(start + 3, qbad)}); short_seq_only++;
            recs.push_back(Spec{"@short_qual", rnd_str(g, start + 3, "ACGTN"), "+", std::string(start - 1, qbad)}); short_qual_only++;
        } else recs.push_back(Spec{"@empty", "", "+", ""});
        // a byte at or above 0x80 in one line only, at the line's first and last byte
        const std::string sq = rnd_str(g, 30, "ACGT"), qq(30, qok);
        recs.push_back(Spec{"@hdr\xC3", sq, "+", qq});
        recs.push_back(Spec{"@seq", "\x80" + sq.substr(2) + "\xFF", "+", qq});
        recs.push_back(Spec{"@qual", sq, "+", "\xFE" + qq.substr(2) + "\x80"});
        recs.push_back(Spec{"@plus", sq, "\x80\xFF+\xC3\xA9", qq});                   // must NOT be flagged
        const uint64_t n_rec = recs.size(), plus_only = n_rec - 1;
        const Fastq f = make_fastq(recs, crlf, false);
        const QualWant w = ref_qual(f, start, cap, quality, ns);
        // what is kept is this mode's own choice: launch_qual_decide and the de-duplication have modes of their own
        std::vector<uint8_t> alive(n_rec), dup(n_rec), want_keep(n_rec); std::vector<uint32_t> want_len(n_rec); uint64_t kept = 0;
        const bool with_dup = combo % 3 != 0, with_keep = combo % 4 != 0;
        std::string want_out;
        for (uint64_t r = 0; r < n_rec; r++) {
            alive[r] = r % 5 != 2 && !(w.flags[r] & QF_SHORT); dup[r] = r % 9 == 4;
            want_keep[r] = alive[r] && !(with_dup && dup[r]); want_len[r] = want_keep[r] ? w.olen[r] : 0; kept += want_keep[r];
            if (want_keep[r]) want_out += rec_out(f.eff[r], w.s[r], w.q[r]);
        }
        const std::vector<uint8_t> want_bytes(want_out.begin(), want_out.end());
        J j("qual");
        uint64_t bad_wrong = 0, flags_wrong = 0, sl_wrong = 0, ql_wrong = 0, olen_wrong = 0, first_wrong = 0, keep_wrong = 0, len_wrong = 0, kept_wrong = 0, out_wrong = 0, plus_flagged = 0;
        for (unsigned off = 0; off < 16; off++) {
            Text tx(f.text, off);
            Dev<uint64_t> d_ls(f.ls.size()); d_ls.put(f.ls);
            Dev<uint32_t> d_bad(n_rec), d_sl(n_rec), d_ql(n_rec), d_olen(n_rec), d_first(1); Dev<uint8_t> d_fl(n_rec);
            d_first.put({~0u});
            CK(launch_qual_scan(tx.p, d_ls.p(), n_rec, start, cap, quality, ns, d_bad.p(), d_fl.p(), d_sl.p(), d_ql.p(), d_olen.p(), d_first.p(), g_st)); sync_st();
            const auto fl = d_fl.get(n_rec);
            bad_wrong += diff(d_bad.get(n_rec), w.bad); flags_wrong += diff(fl, w.flags); sl_wrong += diff(d_sl.get(n_rec), w.cut_sl); ql_wrong += diff(d_ql.get(n_rec), w.cut_ql);
            olen_wrong += diff(d_olen.get(n_rec), w.olen); first_wrong += d_first.get(1)[0] != w.first_flag; plus_flagged += (fl[plus_only] & QF_HIGH) != 0;
            // the kernels behind get the right values, whatever the scan gave
            Dev<uint8_t> d_alive(n_rec), d_dup(n_rec), d_keep(n_rec); d_alive.put(alive); d_dup.put(dup);
            Dev<uint32_t> d_rsl(n_rec), d_rql(n_rec), d_rolen(n_rec), d_len(n_rec); d_rsl.put(w.cut_sl); d_rql.put(w.cut_ql); d_rolen.put(w.olen);
            Dev<unsigned long long> d_kept(1); d_kept.put({5ull});
            CK(launch_qual_keep(n_rec, d_alive.p(), with_dup ? d_dup.p() : nullptr, d_rolen.p(), with_keep ? d_keep.p() : nullptr, d_len.p(), d_kept.p(), g_st)); sync_st();
            if (with_keep) keep_wrong += diff(d_keep.get(n_rec), want_keep); else (void)d_keep.get(0);
            len_wrong += diff(d_len.get(n_rec), want_len); kept_wrong += d_kept.get(1)[0] != kept + 5;
            Dev<uint64_t> d_off(n_rec + 1);
            (void)dev_scan(want_len, d_off);
            Dev<uint32_t> d_wlen(n_rec); d_wlen.put(want_len);
            Dev<uint8_t> d_out(want_bytes.size());
            CK(launch_qual_gather(tx.p, d_ls.p(), n_rec, start, d_rsl.p(), d_rql.p(), d_wlen.p(), d_off.p(), d_out.p(), g_st)); sync_st();
            out_wrong += diff(d_out.get(want_bytes.size()), want_bytes);
        }
        uint64_t n_high = 0, n_short = 0, n_nfail = 0;
        for (uint8_t x : w.flags) { n_high += (x & QF_HIGH) != 0; n_short += (x & QF_SHORT) != 0; n_nfail += (x & QF_NFAIL) != 0; }
        j.u("start", start).u("cap", cap).u("quality", quality).u("ns", ns).u("crlf", crlf).u("n_rec", n_rec).u("with_dup", with_dup).u("with_keep", with_keep).u("offsets", 16)
            .u("flag_high", n_high).u("flag_short", n_short).u("flag_nfail", n_nfail).u("short_seq_only", short_seq_only).u("short_qual_only", short_qual_only)
            .u("first_flag", w.first_flag).u("kept", kept).u("out_bytes", want_bytes.size())
            .u("bad_wrong", bad_wrong).u("flags_wrong", flags_wrong).u("cut_sl_wrong", sl_wrong).u("cut_ql_wrong", ql_wrong).u("olen_wrong", olen_wrong).u("first_flag_wrong", first_wrong)
            .u("plus_line_flagged", plus_flagged).u("keep_wrong", keep_wrong).u("out_len_wrong", len_wrong).u("kept_wrong", kept_wrong).u("out_wrong", out_wrong).emit();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ hash
// SipHash-1-3, keys (0, 0), one message byte at a time (Aumasson & Bernstein's description: c = 1 compression round, d = 3 finalisation rounds)
struct Sip {
    uint64_t v0 = 0x736f6d6570736575ull, v1 = 0x646f72616e646f6dull, v2 = 0x6c7967656e657261ull, v3 = 0x7465646279746573ull, m = 0, len = 0;
    static uint64_t rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
    void round()
    {
        v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32); v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
        v0 += v3; v3 = rotl(v3, 21); v3 ^= v0; v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
    }
    void byte(uint8_t c) { m |= (uint64_t)c << (8 * (len & 7)); len++; if ((len & 7) == 0) { v3 ^= m; round(); v0 ^= m; m = 0; } }
    uint64_t finish() { m |= (len & 0xFF) << 56; v3 ^= m; round(); v0 ^= m; v2 ^= 0xFF; round(); round(); round(); return v0 ^ v1 ^ v2 ^ v3; }
};
static uint64_t ref_hash(const std::string &seq) { Sip h; for (unsigned char c : seq) h.byte(c); h.byte(0xFF); return h.finish(); }
static std::string hex64(uint64_t v) { char b[24]; snprintf(b, sizeof b, "\"%016llx\"", (unsigned long long)v); return b; }

static void mode_hash()
{
    std::mt19937_64 g(8);
    std::vector<size_t> lens; for (size_t l = 0; l <= 40; l++) lens.push_back(l);
    lens.push_back(150); lens.push_back(151); lens.push_back(1000);
    for (uint64_t start : {0ull, 3ull}) {
        std::vector<Spec> recs;
        for (size_t l : lens) for (int rep = 0; rep < 2; rep++) { Spec r; r.h = "@" + rnd_str(g, g() % 7, "xyz"); r.s = rnd_str(g, l + start, "ACGTN"); r.q = std::string(r.s.size(), 'I'); recs.push_back(r); }
        if (start) recs.push_back(Spec{"@short", "AC", "+", "II"});          // QF_SHORT: no cut sequence, cut_sl == 0
        const Fastq f = make_fastq(recs, false, false);
        const uint64_t n_rec = recs.size();
        std::vector<uint32_t> cut_sl(n_rec); std::vector<uint64_t> want(n_rec);
        for (uint64_t r = 0; r < n_rec; r++) {
            const std::string cs = f.eff[r].s.size() >= start ? f.eff[r].s.substr(start) : std::string();
            cut_sl[r] = (uint32_t)cs.size(); want[r] = ref_hash(cs);
        }
        J j("hash");
        uint64_t hash_wrong = 0, cover = 0;
        for (unsigned off = 0; off < 16; off++) {
            Text tx(f.text, off);
            Dev<uint64_t> d_ls(f.ls.size()), d_h(n_rec); d_ls.put(f.ls);
            Dev<uint32_t> d_sl(n_rec); d_sl.put(cut_sl);
            CK(launch_qual_hash(tx.p, d_ls.p(), n_rec, start, d_sl.p(), d_h.p(), g_st)); sync_st();
            const auto got = d_h.get(n_rec);
#ifndef INGEST_KERNEL_CHECK_STUB
            hash_wrong += diff(got, want);
#else
            (void)got;
#endif
            for (uint64_t r = 0; r < n_rec; r++) {                   // alignment of the cut's first byte x bytes behind the last whole block
                const uintptr_t a = reinterpret_cast<uintptr_t>(tx.p + f.ls[4 * r + 1] + (cut_sl[r] ? start : 0));
                cover |= 1ull << ((a & 3) * 8 + (cut_sl[r] & 7));
            }
        }
        j.u("start", start).u("n_rec", n_rec).u("short_records", start ? 1 : 0).u("offsets", 16).u("align_x_tail", cover).u("hash_wrong", hash_wrong).emit();
    }
    // a fixed list, with the values: for the caller's own SipHash
    std::vector<std::string> fixed = {"", "A", "ACGT", "ACGTACG", "ACGTACGT", "ACGTACGTACGTACG", "ACGTACGTACGTACGT", "NNNNNNNNNNNNNNNNNNNNNNN"};
    { std::string s; for (int i = 0; i < 150; i++) s.push_back("ACGT"[(i * i + i / 7) & 3]); fixed.push_back(s); fixed.push_back(s + "T"); }
    std::vector<Spec> recs;
    for (const auto &s : fixed) recs.push_back(Spec{"@f", s, "+", std::string(s.size(), 'I')});
    const Fastq f = make_fastq(recs, false, false);
    std::vector<uint32_t> cut_sl; for (const auto &s : fixed) cut_sl.push_back((uint32_t)s.size());
    J j("hash");
    Text tx(f.text, 5);
    Dev<uint64_t> d_ls(f.ls.size()), d_h(fixed.size()); d_ls.put(f.ls);
    Dev<uint32_t> d_sl(fixed.size()); d_sl.put(cut_sl);
    CK(launch_qual_hash(tx.p, d_ls.p(), fixed.size(), 0, d_sl.p(), d_h.p(), g_st)); sync_st();
    const auto got = d_h.get(fixed.size());
    std::string arr = "[";
    for (size_t i = 0; i < fixed.size(); i++) arr += std::string(i ? "," : "") + "{\"seq\":\"" + fixed[i] + "\",\"device\":" + hex64(got[i]) + ",\"reference\":" + hex64(ref_hash(fixed[i])) + "}";
    j.raw("fixed", arr + "]").emit();
}

// ------------------------------------------------------------------------------------------------------------------------------ decide
static uint64_t ref_cutoff(uint32_t len, float limit)          // the reference's `(len as f32 * limit) as usize`: IEEE single product, saturating, NaN -> 0
{
    const volatile float cf = (float)len * limit;
    if (cf != cf || cf <= 0.0f) return 0;
    if (cf >= 18446744073709551616.0f) return ~0ull;
    return (uint64_t)cf;
}
static void mode_decide()
{
    const float limits[] = {0.0f, 0.1f, 0.2f, 0.25f, 0.99f, 1.0f, -1.0f, nanf(""), 1e30f};
    const uint32_t lens[][2] = {{150, 151}, {151, 150}, {100, 99}, {99, 100}, {0, 0}, {1, 2}, {10, 10}, {16777217, 16777219}, {16777219, 16777217}, {4000000000u, 33554433}};
    for (int pe = 0; pe < 2; pe++) for (int trunc = 0; trunc < 2; trunc++) for (float limit : limits) {
        std::vector<uint32_t> bad1, bad2, sl1, ql1; std::vector<uint8_t> fl1, fl2, want;
        uint64_t on_integer = 0;
        for (const auto &l : lens) {
            const uint64_t cutoff = ref_cutoff(pe ? l[0] : l[1], limit);
            const volatile float cf = (float)(pe ? l[0] : l[1]) * limit;
            on_integer += cf > 0.0f && cf < 1e9f && cf == (float)(uint64_t)cf;          // (150 x 0.2f is 30 in f32 and 30.000000447 exactly)
            for (int d1 = -1; d1 <= 1; d1++) for (int d2 = -1; d2 <= 1; d2++) for (int nf = 0; nf < 3; nf++) {
                auto near_cut = [&](int d) { const uint64_t v = d < 0 ? (cutoff ? cutoff - 1 : 0) : cutoff + (uint64_t)d < cutoff ? ~0ull : cutoff + (uint64_t)d; return (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull); };
                const uint32_t b1 = near_cut(d1), b2 = near_cut(d2);
                const uint8_t f1 = (uint8_t)((nf == 1 ? QF_NFAIL : 0) | (d1 == 0 ? QF_HIGH : 0)), f2 = (uint8_t)((nf == 2 ? QF_NFAIL : 0) | (d2 == 1 ? QF_SHORT : 0));
                bool drop = false;
                if (!trunc) {
                    if (f1 & QF_NFAIL) drop = true;
                    if (pe && (f2 & QF_NFAIL)) drop = true;
                    if ((uint64_t)b1 >= cutoff) drop = true;
                    if (pe && (uint64_t)b2 >= cutoff) drop = true;
                }
                bad1.push_back(b1); bad2.push_back(b2); sl1.push_back(l[0]); ql1.push_back(l[1]); fl1.push_back(f1); fl2.push_back(f2); want.push_back(drop ? 0 : 1);
            }
        }
        const uint64_t n = want.size();
        J j("decide");
        Dev<uint32_t> d_b1(n), d_b2(n), d_sl(n), d_ql(n); Dev<uint8_t> d_f1(n), d_f2(n), d_alive(n);
        d_b1.put(bad1); d_b2.put(bad2); d_sl.put(sl1); d_ql.put(ql1); d_f1.put(fl1); d_f2.put(fl2);
        CK(launch_qual_decide(n, pe, trunc, limit, d_b1.p(), d_f1.p(), d_sl.p(), d_ql.p(), pe ? d_b2.p() : nullptr, pe ? d_f2.p() : nullptr, d_alive.p(), g_st)); sync_st();
        uint64_t n_alive = 0; for (uint8_t a : want) n_alive += a;
        char lim[32]; snprintf(lim, sizeof lim, "%g", limit);
        j.u("pe", pe).u("trunc", trunc).str("limit", lim).u("n", n).u("alive", n_alive).u("product_on_integer", on_integer).u("alive_wrong", diff(d_alive.get(n), want)).emit();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ dedup
// (the product's slot function, mf_kernels.hip, restated only to FIND keys that share a slot of a 16-slot table; no reference value depends on it)
static uint64_t slot_mix(uint64_t x) { x ^= x >> 32; x *= 0xD6E8FEB86659FD93ULL; x ^= x >> 32; return x; }
static void mode_dedup()
{
    std::mt19937_64 g(10);
    std::vector<uint64_t> same;                                          // keys whose home is slot 3 of 16, by the product's slot function and by the low bits
    while (same.size() < 5) { const uint64_t h = g(); if (h && (h & 15) == 3 && (slot_mix(h) & 15) == 3) same.push_back(h); }
    struct Batch { std::vector<uint64_t> h; std::vector<uint8_t> alive; };
    std::vector<Batch> batches;
    auto add = [&](Batch &b, uint64_t h, int alive) { b.h.push_back(h); b.alive.push_back((uint8_t)alive); };
    const uint64_t X = g() | 1, D1 = g() | 1, D2 = g() | 1;
    { Batch b; for (int i = 0; i < 4; i++) add(b, same[i], 1); add(b, same[0], 1); add(b, 0, 0); add(b, 0, 1); add(b, 0, 1); batches.push_back(b); }          // 8 records, 4 keys, 16 slots; the hash 0 dead, then twice alive
    { Batch b; add(b, same[2], 1); add(b, same[4], 0); add(b, same[4], 1); add(b, 0, 0); batches.push_back(b); }                 // a dead record's hash carried by a later live one
    { Batch b;                                                                                                           // hundreds of copies of one hash, and of 0, in one launch
      for (int i = 0; i < 700; i++) { const int k = i % 7; add(b, k < 3 ? X : k == 3 ? 0 : k == 4 ? same[i % 5] : g() | 1, i % 11 != 0); }
      batches.push_back(b); }
    { Batch b; add(b, D1, 0); add(b, D2, 0); add(b, D1, 1); add(b, X, 1); add(b, D1, 1); batches.push_back(b); }                 // D2 stays dead here ...
    { Batch b; add(b, D2, 1); add(b, D2, 1); add(b, 0, 1); for (int i = 0; i < 5000; i++) add(b, i % 3 ? g() | 1 : batches[2].h[g() % 700], i % 13 != 0); batches.push_back(b); }          // ... and lives here
    uint64_t slots = 16, n_keys = 0, base = 0, rehash_with_keys = 0, max_copies = 0;
    Dev<unsigned long long> *keys = new Dev<unsigned long long>(slots), *first = new Dev<unsigned long long>(slots);
    keys->put(std::vector<unsigned long long>(slots, 0)); first->put(std::vector<unsigned long long>(slots, ~0ull));
    Dev<unsigned long long> d_small(2); d_small.put({~0ull, 0ull});          // zero_idx, n_keys
    std::map<uint64_t, uint64_t> want;                                       // hash -> the smallest file index of a live record that carried it
    auto table_wrong = [&]() -> uint64_t {
        const auto k = keys->get(slots); const auto f = first->get(slots);
        std::map<uint64_t, uint64_t> got; uint64_t bad = 0;
        for (uint64_t s = 0; s < slots; s++) { if (!k[s]) { bad += f[s] != ~0ull; continue; } bad += got.count(k[s]); got[k[s]] = f[s]; }
        std::map<uint64_t, uint64_t> w = want; w.erase(0);
        if (got.size() != w.size()) bad += got.size() > w.size() ? got.size() - w.size() : w.size() - got.size();
        for (const auto &e : w) { auto it = got.find(e.first); bad += it == got.end() || it->second != e.second; }
        return bad;
    };
    for (size_t bi = 0; bi < batches.size(); bi++) {
        const Batch &b = batches[bi]; const uint64_t n = b.h.size();
        J j("dedup");
        uint64_t rehash_table_wrong = 0, did = 0;
        while (2 * (n_keys + n) > slots) {                                   // the product's rule (q_dedup_room): never more than half the slots, before or after a batch
            Dev<unsigned long long> *k2 = new Dev<unsigned long long>(slots * 2), *f2 = new Dev<unsigned long long>(slots * 2);
            k2->put(std::vector<unsigned long long>(slots * 2, 0)); f2->put(std::vector<unsigned long long>(slots * 2, ~0ull));
            CK(launch_dedup_rehash(keys->p(), first->p(), slots, k2->p(), f2->p(), slots * 2, g_st)); sync_st();
            (void)keys->get(slots); (void)first->get(slots);
            delete keys; delete first; keys = k2; first = f2; slots *= 2;
            did++; rehash_with_keys += n_keys != 0;
            rehash_table_wrong += table_wrong();
        }
        if (2 * (n_keys + n) > slots) { fprintf(stderr, "driver: the table would pass half full\n"); exit(3); }
        std::vector<uint8_t> want_dup(n, 0); std::map<uint64_t, uint64_t> copies;
        for (uint64_t i = 0; i < n; i++) {
            if (!b.alive[i]) continue;
            max_copies = std::max(max_copies, ++copies[b.h[i]]);
            if (want.count(b.h[i])) want_dup[i] = 1; else want[b.h[i]] = base + i;
        }
        Dev<uint64_t> d_h(n); d_h.put(b.h);
        Dev<uint8_t> d_alive(n), d_dup(n); d_alive.put(b.alive);
        CK(launch_dedup(d_h.p(), d_alive.p(), (uint32_t)n, base, keys->p(), first->p(), slots, d_small.p(), d_small.p() + 1, d_dup.p(), g_st)); sync_st();
        const auto small = d_small.get(2);
        const uint64_t want_zero = want.count(0) ? want[0] : ~0ull, want_keys = want.size() - want.count(0);
        uint64_t n_dup = 0; for (uint8_t d : want_dup) n_dup += d;
        j.u("batch", bi).u("n", n).u("base", base).u("slots", slots).u("keys_before", n_keys).u("keys_after", want_keys).u("rehashes", did).u("rehashes_with_keys", rehash_with_keys)
            .u("same_slot_keys", same.size()).u("max_copies", max_copies).u("duplicates", n_dup).u("zero_seen", want.count(0))
            .u("dup_wrong", diff(d_dup.get(n), want_dup)).u("n_keys_wrong", small[1] != want_keys).u("zero_idx_wrong", small[0] != want_zero)
            .u("table_wrong", table_wrong()).u("rehash_table_wrong", rehash_table_wrong).emit();
        n_keys = want_keys; base += n;
    }
    delete keys; delete first;
}

// ------------------------------------------------------------------------------------------------------------------------------ bytes
static void mode_bytes()
{
    const uint64_t sizes[] = {1, 8, 15, 16, 17, 4096, (1ull << 20) + 3, 1ull << 20};
    const unsigned shifts[][2] = {{0, 0}, {1, 0}, {0, 1}, {3, 5}};          // bytes the source / the destination lie behind a 16-aligned address
    std::mt19937_64 g(11);
    for (uint64_t n : sizes) for (const auto &sh : shifts) for (int to_host = 0; to_host < 2; to_host++) {
        std::vector<uint8_t> data(n); for (auto &c : data) c = (uint8_t)g();
        const size_t room = CAN + 16 + n + SLACK + CAN;
        uint8_t *pin = nullptr; CK(hipHostMalloc(&pin, room, hipHostMallocDefault));
        memset(pin, PAT, room);
        J j("bytes");
        uint64_t wrong = 0;
        if (!to_host) {
            memcpy(pin + CAN + sh[0], data.data(), n);
            Dev<uint8_t> d(n + 16);
            CK(launch_bytes_from_host(d.p() + sh[1], pin + CAN + sh[0], n, g_st)); sync_st();
            std::vector<uint8_t> want(sh[1], PAT); want.insert(want.end(), data.begin(), data.end());
            wrong = diff(d.get(n + sh[1]), want);
        } else {
            Dev<uint8_t> d(n + 16); d.put(data, sh[0]);
            CK(launch_bytes_to_host(pin + CAN + sh[1], d.p() + sh[0], n, g_st)); sync_st();
            for (size_t i = 0; i < room; i++) {
                const bool in = i >= CAN + sh[1] && i < CAN + sh[1] + n;
                if (in) wrong += pin[i] != data[i - CAN - sh[1]]; else g_canary += pin[i] != PAT;
            }
            std::vector<uint8_t> src(sh[0], PAT); src.insert(src.end(), data.begin(), data.end());
            wrong += diff(d.get(n + sh[0]), src);                        // (the source is left alone)
        }
        const bool wide = ((n | sh[0] | sh[1]) & 15) == 0;
        j.str("direction", to_host ? "to_host" : "from_host").u("n", n).u("src_shift", sh[0]).u("dst_shift", sh[1]).str("path", wide ? "uint4" : "byte").u("wrong", wrong);
        CK(hipHostFree(pin));
        j.emit();
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: ingest_kernel_check scan|lines|seqlens|pack|select|qual|hash|decide|dedup|bytes\n"); return 2; }
    const std::string m = argv[1];
    CK(hipSetDevice(0));
    CK(hipStreamCreateWithFlags(&g_st, hipStreamNonBlocking));
    if (m == "scan") mode_scan();
    else if (m == "lines") mode_lines();
    else if (m == "seqlens") mode_seqlens();
    else if (m == "pack") mode_pack();
    else if (m == "select") mode_select();
    else if (m == "qual") mode_qual();
    else if (m == "hash") mode_hash();
    else if (m == "decide") mode_decide();
    else if (m == "dedup") mode_dedup();
    else if (m == "bytes") mode_bytes();
    else { fprintf(stderr, "unknown mode %s\n", m.c_str()); return 2; }
    CK(hipStreamSynchronize(g_st));
    CK(hipStreamDestroy(g_st));
    printf("{\"mode\":\"%s\",\"done\":1}\n", m.c_str());
    return 0;
}
