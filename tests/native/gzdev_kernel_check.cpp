// TEST INFRASTRUCTURE: the kernels of the device DEFLATE decoder (mitoflex_amd/csrc/mf_gzdev.hip) held to zlib, one JSON line per case.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -x hip gzdev_kernel_check.cpp mitoflex_amd/csrc/build/mf_gzdev.o -lz
//   gzdev_kernel_check decode --chunks 1024,4096 [--expansion 8] [--cap SYMBOLS] [--ring BYTES] [--limit BYTES] [--exact-kind stored|fixed|dynamic] FILE.gz...
//   gzdev_kernel_check link SEED...
//   gzdev_kernel_check crc
// decode: launch_gz_decode over every chunk of the (single-member, plain-header) file, then every chunk that starts at a true block boundary
//   -- from zlib's Z_BLOCK mode -- is checked against zlib's text: its symbols (markers resolved from the 32 KiB in front), where and why it
//   stopped.  Then the chunks are linked the way the product links them (gz_link_walk on the host, launch_gz_link + launch_gz_resolve per slab;
//   where the walk meets a gap the host's part is played from zlib's text) and the text and the window left behind are compared with zlib's.
//   --ring: the file goes through a power-of-two ring of that many bytes, slab by slab, each slab decoded with the bytes uploaded so far as its
//   limit; --limit: every chunk is decoded twice, without and with that limit, and the two must agree as the limit's rules say; --exact-kind:
//   the decode starts at the first chunk whose range holds a true boundary in front of a block of that kind (chunk_lo > 0, exact restart there);
//   --cap: symbols of room per chunk (small: OVERFLOW).
// link: the link kernels on synthetic chunks (no DEFLATE): symbols that are bytes or markers into the 32 KiB in front of their chunk, the
//   text and the window they must give.
// crc: launch_gz_crc + gz_crc_finish, and gz_crc_combine, against zlib's crc32.
// Every HIP call is checked: the first error ends the run with exit status 2.  Results are for the caller to judge (the JSON fields).
#include "mf_gzdev.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <map>
#include <random>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>

using namespace mf;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

template <class T> static T *dalloc(size_t n) { T *p = nullptr; CK(hipMalloc(&p, n * sizeof(T) + 64)); return p; }

static std::vector<uint8_t> slurp(const char *p)
{
    std::vector<uint8_t> v; FILE *f = fopen(p, "rb"); if (!f) { perror(p); exit(2); }
    uint8_t b[1 << 16]; size_t n; while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f); return v;
}

// ---------------------------------------------------------------------------------------------------------------------------- decode
struct Truth {
    std::vector<uint8_t> text;
    std::vector<uint64_t> bit, off;      // every block's header (absolute bits of the file) and the text offset there
    uint64_t end_bit = 0;                // the byte behind the final block, in bits
    std::map<uint64_t, size_t> at;       // bit -> index of the block starting there
};

static bool z_truth(const std::vector<uint8_t> &gz, size_t hdr, Truth &t)
{
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    std::vector<uint8_t> obuf(1 << 16);
    t.bit.push_back(hdr * 8); t.off.push_back(0);
    zs.next_in = const_cast<uint8_t *>(gz.data()) + hdr; zs.avail_in = (uInt)(gz.size() - hdr);
    for (;;) {
        zs.next_out = obuf.data(); zs.avail_out = (uInt)obuf.size();
        const int rc = inflate(&zs, Z_BLOCK);
        t.text.insert(t.text.end(), obuf.data(), obuf.data() + (obuf.size() - zs.avail_out));
        if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&zs); return false; }
        const uint64_t bit = (uint64_t)(zs.next_in - gz.data()) * 8 - (uint64_t)(zs.data_type & 7);
        if (rc == Z_STREAM_END) { t.end_bit = bit; break; }
        if ((zs.data_type & 128) && !(zs.data_type & 64) && t.bit.back() != bit) { t.bit.push_back(bit); t.off.push_back(t.text.size()); }
    }
    inflateEnd(&zs);
    for (size_t i = 0; i < t.bit.size(); i++) t.at[t.bit[i]] = i;
    return true;
}

static unsigned block_kind(const std::vector<uint8_t> &gz, uint64_t bit)      // BTYPE of the block whose header starts at `bit`
{
    auto get = [&](uint64_t b) { return (gz[b >> 3] >> (b & 7)) & 1u; };
    return get(bit + 1) | get(bit + 2) << 1;
}

struct DecodeOpts { uint64_t chunk = 4096, expansion = 8, cap = 0, ring = 0, limit = 0; int exact_kind = -1; };

// decode chunks [lo, hi) into d_chunks and h (descriptors, indexed by chunk number) and d_sym (chunk c at (c - lo) * cap); limit / ring as the product passes them
static void run_decode(const std::vector<uint8_t> &gz, size_t hdr, const DecodeOpts &o, uint32_t lo, uint32_t hi, uint32_t exact_chunk, uint64_t exact_bit,
                       uint64_t cap, uint16_t *d_sym, GzChunk *d_chunks, std::vector<GzChunk> &h, uint64_t limit)
{
    const uint64_t size = gz.size(), n = hi - lo;
    uint32_t *d_scr = gz_decode_serial() ? nullptr : dalloc<uint32_t>(gz_decode_scratch_bytes((uint32_t)n) / 4);
    CK(hipMemset(d_chunks, 0xEE, h.size() * sizeof(GzChunk)));
    if (!o.ring) {
        uint8_t *d = dalloc<uint8_t>(size + 256);
        CK(hipMemset(d, 0, size + 256)); CK(hipMemcpy(d, gz.data(), size, hipMemcpyHostToDevice));
        CK(launch_gz_decode(d, 0, size, limit ? limit : size, hdr, o.chunk, lo, (uint32_t)n, exact_chunk, exact_bit, d_sym, cap, d_chunks, d_scr, 0));
        CK(hipDeviceSynchronize());
        CK(hipFree(d));
    } else {
        // slab by slab through the ring: a slab's chunks read their own range, up to a chunk's worth of blocks behind it, and a little more
        const uint64_t R = o.ring, margin = o.chunk + 4096;
        const uint64_t per = std::max<uint64_t>(1, (R - margin - 512) / o.chunk);
        uint8_t *d = dalloc<uint8_t>(R + 4096);
        CK(hipMemset(d, 0xA5, R + 4096));
        uint64_t up_lo = 0, up_hi = 0;          // bytes of the file in the ring: [up_lo, up_hi)
        for (uint32_t s = lo; s < hi; s += (uint32_t)per) {
            const uint32_t e = (uint32_t)std::min<uint64_t>(hi, s + per);
            const uint64_t from = std::min<uint64_t>(s == exact_chunk ? exact_bit / 8 : hdr + (uint64_t)s * o.chunk, size) & ~(uint64_t)255;
            const uint64_t upto = std::min<uint64_t>(size, hdr + (uint64_t)e * o.chunk + margin);
            if (upto - from + 256 > R) { fprintf(stderr, "ring of %llu bytes too small for a slab\n", (unsigned long long)R); exit(2); }
            up_lo = std::max(up_lo, from);
            for (uint64_t b = std::max(up_hi, up_lo); b < upto;) {          // the new bytes, in at most two pieces (the end of the ring)
                const uint64_t r0 = b & (R - 1), k = std::min(upto - b, R - r0);
                CK(hipMemcpy(d + r0, gz.data() + b, k, hipMemcpyHostToDevice)); b += k;
            }
            up_hi = upto;
            if (upto == size) {                     // readable and zero behind the last byte
                const uint64_t z0 = size & (R - 1), zf = std::min<uint64_t>(256, R - z0);
                CK(hipMemset(d + z0, 0, zf)); if (zf < 256) CK(hipMemset(d, 0, 256 - zf));
            }
            const uint64_t lim = limit ? std::min(limit, upto) : upto;
            CK(launch_gz_decode(d, R, size, lim, hdr, o.chunk, s, e - s, exact_chunk, exact_bit, d_sym + (uint64_t)(s - lo) * cap, cap, d_chunks, d_scr, 0));
            CK(hipDeviceSynchronize());
        }
        CK(hipFree(d));
    }
    CK(hipMemcpy(h.data() + lo, d_chunks + lo, n * sizeof(GzChunk), hipMemcpyDeviceToHost));          // (descriptors by chunk number)
    if (d_scr) CK(hipFree(d_scr));
}

static int decode_file(const char *path, const DecodeOpts &o)
{
    std::vector<uint8_t> gz = slurp(path);
    if (gz.size() < 18 || gz[0] != 0x1f || gz[1] != 0x8b || gz[2] != 8 || gz[3] != 0) { fprintf(stderr, "%s: plain 10-byte gzip header expected\n", path); return 2; }
    const size_t hdr = 10;
    Truth t;
    if (!z_truth(gz, hdr, t)) { fprintf(stderr, "%s: zlib does not decode it\n", path); return 2; }
    const uint64_t size = gz.size();
    const uint32_t n_chunks = (uint32_t)((size - hdr + o.chunk - 1) / o.chunk);
    const uint64_t cap = o.cap ? o.cap : o.chunk * o.expansion + 262144;
    const bool serial = gz_decode_serial();
    // where the decode starts: chunk 0 at the member's first block, or an exact restart in front of the first block of the wanted kind behind chunk 0
    uint32_t lo = 0; uint64_t exact_bit = (uint64_t)hdr * 8; int exact_kind = -1;
    if (o.exact_kind >= 0) {
        bool found = false;
        for (size_t i = 1; i < t.bit.size() && !found; i++) {
            const uint32_t c = (uint32_t)((t.bit[i] / 8 - hdr) / o.chunk);
            if (c >= 1 && (int)block_kind(gz, t.bit[i]) == o.exact_kind) { lo = c; exact_bit = t.bit[i]; found = true; }
        }
        if (!found) { printf("{\"file\": \"%s\", \"chunk\": %llu, \"exact_kind\": %d, \"error\": \"no such block behind chunk 0\"}\n", path, (unsigned long long)o.chunk, o.exact_kind); return 0; }
        exact_kind = o.exact_kind;
    }
    const uint32_t n = n_chunks - lo;
    uint16_t *d_sym = dalloc<uint16_t>((size_t)n * cap);
    GzChunk *d_chunks = dalloc<GzChunk>(n_chunks);
    std::vector<GzChunk> h(n_chunks);
    run_decode(gz, hdr, o, lo, n_chunks, lo, exact_bit, cap, d_sym, d_chunks, h, o.ring ? 0 : o.limit);
    // ---- every chunk that starts at a true boundary
    uint32_t hist[5] = {0, 0, 0, 0, 0};
    uint64_t verified = 0, verified_nonfirst = 0, wrong = 0, bad_end = 0, markers = 0, spec_false = 0, overflow_verified = 0;
    uint32_t min_marker = 0xFFFFFFFFu; bool exact_ok = false;
    std::string first_bad;
    std::vector<uint16_t> sym;
    const uint64_t margin = serial ? 1024 : 8;          // what the kernels keep free in the symbol buffer (STG of the one-lane walk; a 16-byte read of the lane kernel)
    for (uint32_t c = lo; c < n_chunks; c++) {
        const GzChunk &k = h[c];
        hist[k.status < 5 ? k.status : 0]++;
        if (k.status != GZ_AT_BOUNDARY && k.status != GZ_MEMBER_END && k.status != GZ_OVERFLOW) continue;
        auto it = t.at.find(k.start_bit);
        if (it == t.at.end()) { spec_false++; continue; }
        const size_t i = it->second; const uint64_t T = t.off[i];
        const uint64_t wrong_before = wrong;
        bool ok = T + k.n_sym <= t.text.size() && k.n_sym <= cap;
        if (ok) {
            sym.resize(k.n_sym);
            if (k.n_sym) CK(hipMemcpy(sym.data(), d_sym + (size_t)(c - lo) * cap, (size_t)k.n_sym * 2, hipMemcpyDeviceToHost));
            for (uint32_t s = 0; s < k.n_sym; s++) {
                const uint16_t v = sym[s];
                uint8_t b;
                if (v & GZ_MARK) {
                    const uint32_t idx = v & 0x7FFF;
                    markers++; min_marker = std::min(min_marker, idx);
                    if (T + idx < GZ_WINDOW || T - GZ_WINDOW + idx >= T + s) { wrong++; continue; }          // in front of the text, or not in front of the chunk
                    b = t.text[T - GZ_WINDOW + idx];
                } else if (v > 255) { wrong++; continue; }
                else b = (uint8_t)v;
                if (b != t.text[T + s]) wrong++;
            }
        } else wrong++;
        // where and why it stopped
        bool end_ok = false;
        // (zlib gives the member's end rounded up to a byte: the end-of-block code of the final block ends in the byte in front of it)
        if (k.status == GZ_MEMBER_END) end_ok = k.end_bit <= t.end_bit && k.end_bit + 8 > t.end_bit && k.end_bit > t.bit.back() && T + k.n_sym == t.text.size();
        else {
            auto e = t.at.find(k.end_bit);
            if (e != t.at.end() && e->second >= i && t.off[e->second] - T == k.n_sym) {
                end_ok = true;
                if (k.status == GZ_OVERFLOW) {              // the block behind end_bit did not fit
                    const uint64_t next_off = e->second + 1 < t.off.size() ? t.off[e->second + 1] : t.text.size();
                    end_ok = next_off - T + margin > cap;
                }
            }
        }
        if (!end_ok) bad_end++;
        if ((!end_ok || wrong != wrong_before) && first_bad.empty()) {
            char b[200]; snprintf(b, sizeof b, "chunk %u status %u start %llu end %llu n_sym %u", c, k.status, (unsigned long long)k.start_bit, (unsigned long long)k.end_bit, k.n_sym);
            first_bad = b;
        }
        verified++;
        if (c != lo) verified_nonfirst++;
        if (k.status == GZ_OVERFLOW && end_ok) overflow_verified++;
        if (c == lo && k.start_bit == exact_bit) exact_ok = true;
    }
    if (h[lo].status == GZ_FAILED || h[lo].start_bit != exact_bit) exact_ok = false;
    // ---- the limit's rules: the same chunks once more without a limit (or, through the ring, with the whole file as the limit)
    uint64_t limit_violations = 0;
    if (o.limit) {
        DecodeOpts full = o; full.ring = 0; full.limit = 0;
        std::vector<GzChunk> f(n_chunks);
        uint16_t *d_sym2 = dalloc<uint16_t>((size_t)n * cap);
        run_decode(gz, hdr, full, lo, n_chunks, lo, exact_bit, cap, d_sym2, d_chunks, f, 0);
        CK(hipFree(d_sym2));
        for (uint32_t c = lo; c < n_chunks; c++) {
            const GzChunk &a = h[c], &b = f[c];
            const bool a_ok = a.status == GZ_AT_BOUNDARY || a.status == GZ_MEMBER_END || a.status == GZ_OVERFLOW;
            const bool b_ok = b.status == GZ_AT_BOUNDARY || b.status == GZ_MEMBER_END || b.status == GZ_OVERFLOW;
            if (a_ok && (a.end_bit > o.limit * 8 || a.start_bit != b.start_bit || a.end_bit != b.end_bit || a.n_sym != b.n_sym || a.status != b.status)) limit_violations++;
            if (b_ok && b.end_bit > o.limit * 8 && !(a.status == GZ_FAILED && a.n_sym == 8)) limit_violations++;
            if (a.status == GZ_FAILED && a.n_sym == 8 && b_ok && b.end_bit <= o.limit * 8 && t.at.count(b.start_bit) && c == lo) limit_violations++;
        }
    }
    // ---- link the way the product does; where the walk stops at a gap, the host's part (inflate_gap) is played from zlib's text
    const uint32_t slab = 512;
    uint8_t *d_text = dalloc<uint8_t>(t.text.size() + GZ_WINDOW + 256);
    uint8_t *d_window = dalloc<uint8_t>(GZ_WINDOW);
    uint8_t *d_link = dalloc<uint8_t>(gz_link_scratch_bytes(slab));
    uint32_t *d_acc = dalloc<uint32_t>(slab); uint64_t *d_acc_off = dalloc<uint64_t>(slab);
    uint8_t *text0 = d_text + GZ_WINDOW + 256;          // text offset 0 (room for a window in front of it)
    CK(hipMemset(d_text, 0, t.text.size() + GZ_WINDOW + 256)); CK(hipMemset(d_window, 0, GZ_WINDOW));
    GzLinkState st; st.cur_bit = exact_bit; st.total = t.off[t.at[exact_bit]]; st.next = lo;
    st.wlen = (uint32_t)std::min<uint64_t>(st.total, GZ_WINDOW);
    auto put_window = [&](uint64_t total) {           // the host's window and text up to `total` (what a gap fill leaves on the device)
        const uint64_t w = std::min<uint64_t>(total, GZ_WINDOW);
        if (w) CK(hipMemcpy(d_window + GZ_WINDOW - w, t.text.data() + total - w, w, hipMemcpyHostToDevice));
    };
    put_window(st.total);
    if (st.total) CK(hipMemcpy(text0, t.text.data(), st.total, hipMemcpyHostToDevice));
    uint64_t linked_chunks = 0, linked_bytes = 0, bridged_bytes = 0, gaps = 0, accepted_not_true = 0, link_calls = 0;
    std::vector<uint32_t> acc; std::vector<uint64_t> acc_off;
    bool member_end = false, link_overrun = false;
    for (uint32_t s = lo; s < n_chunks && !member_end;) {
        const uint32_t e = std::min<uint32_t>(n_chunks, s + slab);
        if (st.next < s) st.next = s;
        const uint32_t wlen_before = st.wlen;
        gz_link_walk(h.data(), e, st, acc, acc_off);
        if (!acc.empty() && acc_off.back() + h[acc.back()].n_sym > t.text.size()) { link_overrun = true; break; }      // (more text than zlib's: not written anywhere)
        if (!acc.empty()) {
            uint32_t mx = 0;
            for (size_t j = 0; j < acc.size(); j++) {
                mx = std::max(mx, h[acc[j]].n_sym);
                if (!t.at.count(h[acc[j]].start_bit) || t.off[t.at[h[acc[j]].start_bit]] != acc_off[j]) accepted_not_true++;
            }
            // (chunk numbers relative to the slab's first chunk, as the product passes them)
            CK(hipMemcpy(d_acc, acc.data(), acc.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_acc_off, acc_off.data(), acc_off.size() * 8, hipMemcpyHostToDevice));
            CK(launch_gz_link(d_acc, d_acc_off, (uint32_t)acc.size(), mx, d_chunks, s, d_sym + (size_t)(s - lo) * cap, cap, d_window, wlen_before, d_link, text0, 0, acc_off[0], 0));
            CK(launch_gz_resolve(d_acc, d_acc_off, (uint32_t)acc.size(), mx, d_chunks, s, d_sym + (size_t)(s - lo) * cap, cap, text0, 0, 0));
            CK(hipDeviceSynchronize());
            linked_chunks += acc.size(); link_calls++;
            for (uint32_t c : acc) linked_bytes += h[c].n_sym;
        }
        if (st.stop == GZ_STOP_MEMBER_END) { member_end = true; break; }
        if (st.stop == GZ_STOP_GAP) {
            // the host decodes from cur_bit to the start of chunk `next` if that is a true boundary; a chunk that is not is passed over
            const GzChunk &k = h[st.next];
            auto it = t.at.find(k.start_bit);
            if (it == t.at.end()) { st.discarded++; st.next++; continue; }
            const uint64_t to = t.off[it->second];
            if (to > st.total) CK(hipMemcpy(text0 + st.total, t.text.data() + st.total, to - st.total, hipMemcpyHostToDevice));
            bridged_bytes += to - st.total; gaps++;
            st.total = to; st.cur_bit = k.start_bit; st.wlen = (uint32_t)std::min<uint64_t>(to, GZ_WINDOW);
            put_window(to);
            continue;
        }
        s = e;
    }
    // behind the last linked chunk the host decodes to the member's end
    if (link_overrun) st.total = 0;
    if (!member_end && !link_overrun && st.total < t.text.size()) {
        bridged_bytes += t.text.size() - st.total;
        CK(hipMemcpy(text0 + st.total, t.text.data() + st.total, t.text.size() - st.total, hipMemcpyHostToDevice));
        put_window(t.text.size());
        st.total = t.text.size();
    }
    std::vector<uint8_t> got(st.total);
    if (st.total) CK(hipMemcpy(got.data(), text0, st.total, hipMemcpyDeviceToHost));
    const uint64_t T0 = t.off[t.at[exact_bit]];
    uint64_t text_wrong = st.total != t.text.size() || link_overrun;
    for (uint64_t i = T0; i < std::min<uint64_t>(st.total, t.text.size()); i++) text_wrong += got[i] != t.text[i];
    std::vector<uint8_t> w(GZ_WINDOW);
    CK(hipMemcpy(w.data(), d_window, GZ_WINDOW, hipMemcpyDeviceToHost));
    uint64_t window_wrong = 0;
    const uint64_t wl = std::min<uint64_t>(t.text.size(), GZ_WINDOW);
    for (uint64_t i = 0; i < wl; i++) window_wrong += w[GZ_WINDOW - wl + i] != t.text[t.text.size() - wl + i];
    printf("{\"file\": \"%s\", \"chunk\": %llu, \"kernel\": \"%s\", \"ring\": %llu, \"limit\": %llu, \"cap\": %llu, \"exact_kind\": %d, \"chunk_lo\": %u, "
           "\"chunks\": %u, \"blocks\": %zu, \"hist\": [%u, %u, %u, %u, %u], \"verified\": %llu, \"verified_nonfirst\": %llu, \"spec_false\": %llu, "
           "\"wrong\": %llu, \"bad_end\": %llu, \"overflow_verified\": %llu, \"exact_ok\": %s, \"exact_past_limit\": %s, \"markers\": %llu, \"min_marker\": %d, "
           "\"limit_violations\": %llu, \"accepted_not_true\": %llu, \"linked_chunks\": %llu, \"linked_bytes\": %llu, \"link_calls\": %llu, \"gaps\": %llu, "
           "\"bridged_bytes\": %llu, \"member_end_linked\": %s, \"text_bytes\": %zu, \"text_wrong\": %llu, \"window_wrong\": %llu, \"first_bad\": \"%s\"}\n",
           path, (unsigned long long)o.chunk, serial ? "serial" : "lanes", (unsigned long long)o.ring, (unsigned long long)o.limit, (unsigned long long)cap, exact_kind, lo,
           n_chunks, t.bit.size(), hist[0], hist[1], hist[2], hist[3], hist[4], (unsigned long long)verified, (unsigned long long)verified_nonfirst, (unsigned long long)spec_false,
           (unsigned long long)wrong, (unsigned long long)bad_end, (unsigned long long)overflow_verified, exact_ok ? "true" : "false", h[lo].status == GZ_FAILED && h[lo].n_sym == 8 ? "true" : "false", (unsigned long long)markers,
           min_marker == 0xFFFFFFFFu ? -1 : (int)min_marker, (unsigned long long)limit_violations, (unsigned long long)accepted_not_true, (unsigned long long)linked_chunks,
           (unsigned long long)linked_bytes, (unsigned long long)link_calls, (unsigned long long)gaps, (unsigned long long)bridged_bytes, member_end ? "true" : "false", t.text.size(),
           (unsigned long long)text_wrong, (unsigned long long)window_wrong, first_bad.c_str());
    fflush(stdout);
    CK(hipFree(d_sym)); CK(hipFree(d_chunks)); CK(hipFree(d_text)); CK(hipFree(d_window)); CK(hipFree(d_link)); CK(hipFree(d_acc)); CK(hipFree(d_acc_off));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------- link
// One case: n_acc accepted chunks (chunk numbers with passed-over ones between them), wlen_before bytes of window, text addressed from text_base.
static void link_case(uint64_t seed, uint32_t n_acc, uint32_t wlen_before, bool small_only, uint64_t text_base_abs)
{
    std::mt19937_64 rng(seed * 1000003 + n_acc * 7 + wlen_before + (small_only ? 1 : 0));
    static const uint32_t special[] = {0, 1, 100, 32767, 32768, 32769, 100000};
    // text: absolute offsets from A0 = the start of the valid text; the window holds [A0, F) with F = A0 + wlen_before
    const uint64_t A0 = text_base_abs, F = A0 + wlen_before;
    std::vector<uint32_t> nsym(n_acc);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_acc; k++) {
        uint32_t v = rng() % 3 == 0 ? special[rng() % 7] : (uint32_t)(rng() % 6000);
        if (small_only && v > GZ_WINDOW) v = GZ_WINDOW - (uint32_t)(rng() % 2);
        if (total > (8u << 20) && v > 1000) v = (uint32_t)(rng() % 1000);
        nsym[k] = v; total += v;
    }
    uint32_t max_sym = 0; for (uint32_t v : nsym) max_sym = std::max(max_sym, v);
    const uint64_t cap = (max_sym + 15) & ~(uint64_t)7;
    std::vector<uint8_t> text(wlen_before + total);           // text[i] = byte at absolute offset A0 + i
    for (uint32_t i = 0; i < wlen_before; i++) text[i] = (uint8_t)rng();
    const uint32_t chunk_lo = 5;
    std::vector<uint32_t> acc(n_acc); std::vector<uint64_t> acc_off(n_acc);
    uint32_t c = chunk_lo + (uint32_t)(rng() % 3);
    for (uint32_t k = 0; k < n_acc; k++) { acc[k] = c; c += 1 + (rng() % 5 == 0 ? 1 + (uint32_t)(rng() % 2) : 0); }
    const uint32_t n_slots = c - chunk_lo;
    std::vector<uint16_t> sym((size_t)n_slots * cap, 0x7777);
    std::vector<GzChunk> ch(n_slots + chunk_lo);
    for (auto &x : ch) { x.start_bit = 0; x.end_bit = 0; x.n_sym = 0xFFFFFFFFu; x.status = GZ_FAILED; }
    uint64_t pos = wlen_before;                                // index into text of the next chunk's first byte
    uint64_t n_markers = 0, far_markers = 0;
    for (uint32_t k = 0; k < n_acc; k++) {
        acc_off[k] = A0 + pos;
        GzChunk &d = ch[acc[k]];
        d.start_bit = 1000 + k; d.end_bit = 1001 + k; d.n_sym = nsym[k]; d.status = k + 1 == n_acc ? GZ_MEMBER_END : GZ_AT_BOUNDARY;
        uint16_t *sp = sym.data() + (size_t)(acc[k] - chunk_lo) * cap;
        const uint64_t valid_front = std::min<uint64_t>(pos, GZ_WINDOW);          // text in front of the chunk a marker may reach
        const uint32_t mode = (uint32_t)(rng() % 4);                              // 0: bytes only, 1: mostly markers, 2/3: a mix
        for (uint32_t s = 0; s < nsym[k]; s++) {
            const bool mark = valid_front && mode != 0 && (mode == 1 ? rng() % 8 != 0 : rng() % 2 == 0);
            if (mark) {
                const uint32_t lo_idx = (uint32_t)(GZ_WINDOW - valid_front);
                const uint32_t idx = rng() % 4 == 0 ? lo_idx + (uint32_t)(rng() % 8) % (GZ_WINDOW - lo_idx) : lo_idx + (uint32_t)(rng() % (GZ_WINDOW - lo_idx));
                sp[s] = (uint16_t)(GZ_MARK | idx);
                text[pos + s] = text[pos - GZ_WINDOW + idx];
                n_markers++; if (idx < 262) far_markers++;
            } else { const uint8_t b = (uint8_t)rng(); sp[s] = b; text[pos + s] = b; }
        }
        pos += nsym[k];
    }
    // device buffers: text addressed by absolute offset - text_base, with the window's room in front of F
    const uint64_t text_base = F - GZ_WINDOW - 64;
    const size_t text_room = GZ_WINDOW + 64 + total + 64;
    uint8_t *d_text = dalloc<uint8_t>(text_room), *d_window = dalloc<uint8_t>(GZ_WINDOW), *d_link = dalloc<uint8_t>(gz_link_scratch_bytes(n_acc));
    uint16_t *d_sym = dalloc<uint16_t>(sym.size());
    GzChunk *d_ch = dalloc<GzChunk>(ch.size());
    uint32_t *d_acc = dalloc<uint32_t>(n_acc); uint64_t *d_acc_off = dalloc<uint64_t>(n_acc);
    CK(hipMemset(d_text, 0x5A, text_room));
    std::vector<uint8_t> win0(GZ_WINDOW, 0xC3);
    if (wlen_before) memcpy(win0.data() + GZ_WINDOW - wlen_before, text.data(), wlen_before);
    CK(hipMemcpy(d_window, win0.data(), GZ_WINDOW, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_sym, sym.data(), sym.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_ch, ch.data(), ch.size() * sizeof(GzChunk), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_acc, acc.data(), n_acc * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_acc_off, acc_off.data(), n_acc * 8, hipMemcpyHostToDevice));
    // slabs at random points (one slab for n_acc at the group-size edges every other seed, so that the group size is that of n_acc)
    std::vector<uint32_t> cuts = {0};
    if (seed % 2 == 0) for (uint32_t k = 1; k < n_acc; k++) if (rng() % (n_acc / 3 + 2) == 0) cuts.push_back(k);
    cuts.push_back(n_acc);
    uint64_t wlen = wlen_before;
    uint32_t groups_seen = 0;
    for (size_t j = 0; j + 1 < cuts.size(); j++) {
        const uint32_t a = cuts[j], b = cuts[j + 1];
        uint32_t mx = 0; for (uint32_t k = a; k < b; k++) mx = std::max(mx, nsym[k]);
        CK(launch_gz_link(d_acc + a, d_acc_off + a, b - a, mx, d_ch, chunk_lo, d_sym, cap, d_window, (uint32_t)wlen, d_link, d_text, text_base, acc_off[a], 0));
        CK(launch_gz_resolve(d_acc + a, d_acc_off + a, b - a, mx, d_ch, chunk_lo, d_sym, cap, d_text, text_base, 0));
        CK(hipDeviceSynchronize());
        groups_seen |= 1u << (gz_link_group(b - a) == 4 ? 0 : gz_link_group(b - a) == 8 ? 1 : gz_link_group(b - a) == 16 ? 2 : 3);
        for (uint32_t k = a; k < b; k++) wlen = std::min<uint64_t>(wlen + nsym[k], GZ_WINDOW);
    }
    std::vector<uint8_t> got(text_room);
    CK(hipMemcpy(got.data(), d_text, text_room, hipMemcpyDeviceToHost));
    uint64_t text_wrong = 0;
    const uint64_t t0 = F - text_base;              // index in d_text of absolute offset F
    for (uint64_t i = 0; i < total; i++) text_wrong += got[t0 + i] != text[wlen_before + i];
    for (uint64_t i = 0; i < wlen_before; i++) text_wrong += got[t0 - wlen_before + i] != text[i];         // the window in front, written as text
    std::vector<uint8_t> w(GZ_WINDOW);
    CK(hipMemcpy(w.data(), d_window, GZ_WINDOW, hipMemcpyDeviceToHost));
    const uint64_t wl = std::min<uint64_t>(text.size(), GZ_WINDOW);
    uint64_t window_wrong = 0;
    for (uint64_t i = 0; i < wl; i++) window_wrong += w[GZ_WINDOW - wl + i] != text[text.size() - wl + i];
    printf("{\"seed\": %llu, \"n_acc\": %u, \"group\": %u, \"groups_seen\": %u, \"slabs\": %zu, \"wlen_before\": %u, \"max_sym\": %u, \"text_base\": %llu, \"text_bytes\": %llu, "
           "\"markers\": %llu, \"far_markers\": %llu, \"text_wrong\": %llu, \"window_wrong\": %llu}\n",
           (unsigned long long)seed, n_acc, gz_link_group(n_acc), groups_seen, cuts.size() - 1, wlen_before, max_sym, (unsigned long long)text_base, (unsigned long long)total,
           (unsigned long long)n_markers, (unsigned long long)far_markers, (unsigned long long)text_wrong, (unsigned long long)window_wrong);
    fflush(stdout);
    CK(hipFree(d_text)); CK(hipFree(d_window)); CK(hipFree(d_link)); CK(hipFree(d_sym)); CK(hipFree(d_ch)); CK(hipFree(d_acc)); CK(hipFree(d_acc_off));
}

// ---------------------------------------------------------------------------------------------------------------------------- crc
static void crc_cases()
{
    std::mt19937_64 rng(17);
    const uint64_t lens[] = {1, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537, 3 * 65536 + 4095, 10000000 + 7};
    const uint64_t offs[] = {0, 1, 2, 3, 4, 5, 6, 7, 13, 4093};
    const uint64_t big = 10000000 + 7 + 4096 + 64;
    std::vector<uint8_t> buf(big);
    uint8_t *d = dalloc<uint8_t>(big);
    uint32_t *d_piece = dalloc<uint32_t>(big / GZ_CRC_PIECE + 2);
    std::vector<uint32_t> piece(big / GZ_CRC_PIECE + 2);
    uint64_t cases = 0, wrong = 0;
    for (int fill = 0; fill < 3; fill++) {
        for (auto &b : buf) b = fill == 0 ? (uint8_t)rng() : fill == 1 ? 0 : 0xFF;
        CK(hipMemcpy(d, buf.data(), big, hipMemcpyHostToDevice));
        for (uint64_t n : lens)
            for (uint64_t off : offs) {
                if (n > 1000000 && off != 0 && off != 13) continue;
                CK(launch_gz_crc(d + off, n, d_piece, 0));
                const uint64_t np = (n + GZ_CRC_PIECE - 1) / GZ_CRC_PIECE;
                CK(hipMemcpy(piece.data(), d_piece, np * 4, hipMemcpyDeviceToHost));
                const uint32_t got = gz_crc_finish(piece.data(), n);
                const uint32_t want = (uint32_t)crc32(0, buf.data() + off, (uInt)n);
                cases++;
                if (got != want) { wrong++; fprintf(stderr, "crc: fill %d, %llu bytes at +%llu: %08x, zlib %08x\n", fill, (unsigned long long)n, (unsigned long long)off, got, want); }
            }
    }
    // combine: crc32(A || B) from crc32(A), crc32(B), |B| -- |B| = 0 too, and lengths of 2^32 and more (zlib's crc32_combine, 64-bit z_off_t)
    uint64_t comb = 0, comb_wrong = 0;
    for (uint64_t la : {0ull, 1ull, 5000ull, 70000ull})
        for (uint64_t lb : {0ull, 1ull, 7ull, 65536ull, 100001ull}) {
            const uint32_t a = (uint32_t)crc32(0, buf.data(), (uInt)la), b = (uint32_t)crc32(0, buf.data() + la, (uInt)lb);
            const uint32_t ab = (uint32_t)crc32(0, buf.data(), (uInt)(la + lb));
            comb++; if (gz_crc_combine(a, b, lb) != ab) comb_wrong++;
        }
    static_assert(sizeof(z_off_t) >= 8, "64-bit z_off_t");
    for (uint64_t lb : {(1ull << 32) - 1, 1ull << 32, (1ull << 32) + 7, (1ull << 40) + 12345, 0xFFFFFFFFFFFull}) {
        const uint32_t a = (uint32_t)rng(), b = (uint32_t)rng();
        comb++; if (gz_crc_combine(a, b, lb) != (uint32_t)crc32_combine(a, b, (z_off_t)lb)) comb_wrong++;
    }
    printf("{\"crc_cases\": %llu, \"crc_wrong\": %llu, \"combine_cases\": %llu, \"combine_wrong\": %llu}\n", (unsigned long long)cases, (unsigned long long)wrong,
           (unsigned long long)comb, (unsigned long long)comb_wrong);
    CK(hipFree(d)); CK(hipFree(d_piece));
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s decode|link|crc ...\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    if (mode == "crc") { crc_cases(); return 0; }
    if (mode == "link") {
        static const uint32_t n_accs[] = {1, 4, 5, 16, 17, 64, 65, 512, 513};
        for (int a = 2; a < argc; a++) {
            const uint64_t seed = strtoull(argv[a], nullptr, 10);
            for (uint32_t n_acc : n_accs) {
                // (text_base = 0 where the valid text starts at GZ_WINDOW + 64 - wlen_before: the window's room in front of it)
                link_case(seed, n_acc, GZ_WINDOW, false, seed % 2 ? (5ull << 32) + 12345 : 64);
                const uint32_t wl = (uint32_t)(seed * 7919 % GZ_WINDOW);
                link_case(seed, n_acc, wl, n_acc % 2 == 1, seed % 2 ? GZ_WINDOW + 64 - wl : 40000 + seed);
            }
            link_case(seed, 3, 0, true, GZ_WINDOW + 64);           // no text in front at all: bytes only in the first chunk
        }
        return 0;
    }
    if (mode != "decode") { fprintf(stderr, "unknown mode %s\n", argv[1]); return 2; }
    DecodeOpts o;
    std::vector<uint64_t> chunks;
    std::vector<const char *> files;
    for (int a = 2; a < argc; a++) {
        const std::string s = argv[a];
        auto val = [&]() { if (a + 1 >= argc) { fprintf(stderr, "%s needs a value\n", s.c_str()); exit(2); } return std::string(argv[++a]); };
        if (s == "--chunks") { std::string v = val(); for (size_t p = 0; p < v.size();) { size_t q = v.find(',', p); if (q == std::string::npos) q = v.size(); chunks.push_back(strtoull(v.substr(p, q - p).c_str(), nullptr, 10)); p = q + 1; } }
        else if (s == "--expansion") o.expansion = strtoull(val().c_str(), nullptr, 10);
        else if (s == "--cap") o.cap = strtoull(val().c_str(), nullptr, 10);
        else if (s == "--ring") o.ring = strtoull(val().c_str(), nullptr, 10);
        else if (s == "--limit") o.limit = strtoull(val().c_str(), nullptr, 10);
        else if (s == "--exact-kind") { const std::string k = val(); o.exact_kind = k == "stored" ? 0 : k == "fixed" ? 1 : k == "dynamic" ? 2 : -1; if (o.exact_kind < 0) return 2; }
        else files.push_back(argv[a]);
    }
    if (o.ring && (o.ring & (o.ring - 1))) { fprintf(stderr, "--ring: a power of two\n"); return 2; }
    if (chunks.empty()) chunks.push_back(4096);
    for (const char *f : files)
        for (uint64_t c : chunks) { o.chunk = c; const int rc = decode_file(f, o); if (rc) return rc; }
    return 0;
}
