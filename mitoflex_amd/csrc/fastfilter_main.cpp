// `fastfilter` drop-in for MitoFlex (installed as mitoflex_amd/assemble/fastfilter,
// the path MEGAHIT.FAST_FILTER resolves: assemble/assemble_wrapper.py:105-108).
//
// Personality 1 -- the reference's contig filter, argument for argument and
// quirk for quirk (assemble/fastfilter_src/src/main.rs:9-134, helper.rs:12-41):
//     fastfilter -i IN -o OUT -l MIN,MAX (-d INT | -m INT)
// stdout carries the kept count and nothing else (the caller does int(stdout),
// assemble_wrapper.py:326-339); a Rust panic is mirrored as exit code 101, a
// clap usage error as exit code 1.  This part is plain host C++: it is a
// kB-MB text filter and the reference itself is single-threaded host code.
//
// Personality 2 -- the read pre-filter the north star adds (no reference
// counterpart):
//     fastfilter bait --bait BAIT.fa -k 31 [-t 1] --fq1 R1.fq [--fq2 R2.fq]
//                     --out1 O1.fq [--out2 O2.fq] [--pair either|both] [--devices N]
//                     [--report FILE | --group-report FILE [--group-field N] [--group-sep C]
//                      | --depth-report FILE [--depth-profile FILE] | --place-report FILE [--base-depth FILE]
//                      | [--pileup FILE] [--consensus FILE] [--variants FILE] [--min-depth N]]
//                      [--score-report FILE] [--max-mismatch PERMILLE] [--write passing|accepted|placed]
// which loads libmitofilter_hip.so (HIP kernels, gfx950) and prints the kept
// read/pair count.  --report writes how many kept reads (mates one by one)
// each bait record attracted as a TSV (record, name, reads; then the
// ambiguous and the unassigned reads); the FASTQ outputs are the same.  --group-report does the same per group of records
// (group, name, reads), for protein baits too: the records themselves, or with --group-field N the N-th --group-sep separated
// field of the record name (default separator '_'; MT_database headers by gene: --group-field 4).  --depth-report and --depth-profile
// (either alone, for protein baits too) write the K-MER depth of the bait records over every mate that passes its own threshold: per
// record (record, name, length, valid windows, covered windows, mean and max k-mer depth), and per valid window (name, 1-based window
// start in the record, depth: the three columns of `samtools depth -aa`, but k-mer depth, not base depth; include/mitofilter.h,
// mf_depth).  --place-report and --base-depth (either alone, nucleotide baits) write where the passing mates lie on the bait: per record
// (record, name, length, reads placed forward and reverse, reads hanging over its begin and its end, covered positions, mean and max base
// depth, and a last line for the passing mates that are not placed), and per position (name, 1-based position, depth: the columns and
// rows of `samtools depth -aa`; include/mitofilter.h, mf_place).  --pileup, --consensus and --variants (any of them alone, nucleotide
// baits) write what the placed mates' bases say: per position (name, 1-based position, bait letter, depth = A + C + G + T, A, C, G, T,
// in the bait's forward letters), the consensus as FASTA under the bait's record names (called letters in upper case, N where the most
// is tied, the bait's own letter in lower case below --min-depth, default 1), and the called positions that differ from the bait (name,
// 1-based position, ref, alt, depth, alt count; include/mitofilter.h, mf_pileup).  --score-report (alone or with
// either of those two families) writes per record the placed reads' agreement with the bait along their placement: accepted, rejected,
// compared, mismatches, mismatches per thousand, and a histogram of mismatches per read; --max-mismatch PERMILLE (with one of the two
// families or with --score-report, 0 .. 1000) keeps every placed read with more mismatches per thousand compared bases out of the base depth, the placement
// counts and the pile-up (include/mitofilter.h, mf_verify; the output FASTQ files are not changed by it).  --write accepted|placed
// (nucleotide baits; alone or with the placement, pile-up or score reports; default passing) lets that cut decide what is WRITTEN too:
// `accepted` takes the pass bit from every mate that is placed and rejected before the pair rule looks at it, `placed` also from every
// passing mate that is not placed; it makes the call a verifying one by itself, cutting at 1000 unless --max-mismatch is given, and the
// count on stdout is what was written (include/mitofilter.h, the keep rule; the reports do not depend on it).  With --band W,
// --gapped-consensus writes the consensus that calls deletions and insertions too, as FASTA under the bait's record names, and --insertions
// the letters of the inserted bases (name, 1-based position, offset inside the insertion behind it, base depth, A, C, G, T; include/mitofilter.h,
// gapped consensus); without either no call changes.  With --band W --extend E, --extended-consensus writes every record's gapped consensus
// between the columns that the reads overhanging its ends agree on, up to E a side, as FASTA, and --extension-report the overhanging bases
// (name, begin or end, 1-based distance from the record, depth, A, C, G, T; include/mitofilter.h, extended records); without the three flags
// no call changes.  It has no CPU fallback: without the library or a GPU it exits non-zero, which shell_call turns into a RuntimeError
// (helper.py:82-86).
#include "../../include/mitofilter.h"
#include "mf_coldtrace.h"
#include "mf_report_text.h"

#include <dlfcn.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

// ------------------------------------------------------------ error exits
static void (*g_flush_on_panic)() = nullptr;   // BufWriter::drop flushes while the panic unwinds

[[noreturn]] static void rust_panic(const std::string &msg)
{   // mirrors `panic!`/`unwrap()` failures: message on stderr, exit code 101
    if (g_flush_on_panic) { void (*f)() = g_flush_on_panic; g_flush_on_panic = nullptr; f(); }
    fflush(stdout);
    fprintf(stderr, "thread 'main' panicked at '%s'\n", msg.c_str());
    exit(101);
}

static const char *USAGE = "USAGE:\n    fastfilter [OPTIONS] -i <PATH> -l <INT,INT> -o <PATH>\n\nFor more information try --help\n";

[[noreturn]] static void clap_error(const std::string &msg)
{   // clap 2.33 usage errors exit with code 1
    fprintf(stderr, "error: %s\n\n%s", msg.c_str(), USAGE);
    exit(1);
}

static void print_help()
{
    fputs("Length filter 0.1\nJunyu Li\nA simple filter for trimming intermediate contigs.\n\n"
          "USAGE:\n    fastfilter [OPTIONS] -i <PATH> -l <INT,INT> -o <PATH>\n\n"
          "FLAGS:\n    -h, --help       Prints help information\n    -V, --version    Prints version information\n\n"
          "OPTIONS:\n"
          "    -m <INT>            Use it to take only x sequence with highest depth.\n"
          "    -d <INT>            min depth\n"
          "    -i <PATH>           Input file path, accepts only one-line format\n"
          "    -l <INT,INT>        required min and max length\n"
          "    -o <PATH>           Output file path\n", stdout);
}

// ------------------------------------------------------------ Rust parsers
// str::parse::<usize>: optional '+', then ASCII digits only, no overflow
static bool parse_usize(const std::string &s, uint64_t &out)
{
    size_t i = 0;
    if (i < s.size() && s[i] == '+') i++;
    if (i >= s.size()) return false;
    uint64_t v = 0;
    for (; i < s.size(); i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    out = v;
    return true;
}

// str::parse::<i32>: optional sign, digits, range checked
static bool parse_i32(const std::string &s, int32_t &out)
{
    size_t i = 0; bool neg = false;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    if (i >= s.size()) return false;
    int64_t v = 0;
    for (; i < s.size(); i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (s[i] - '0');
        if (v > (int64_t)INT32_MAX + 1) return false;
    }
    if (neg) v = -v;
    if (v < INT32_MIN || v > INT32_MAX) return false;
    out = (int32_t)v;
    return true;
}

// str::parse::<f32> as the shipped binary does it (goldens X14-X17): [sign] then exactly "inf" or
// "NaN", or (digits [. digits] | . digits) [(e|E) [sign] digits]; no surrounding whitespace, no hex,
// no "infinity"/"nan".  Value correctly rounded to binary32 (strtof does the same).
static bool parse_f32(const std::string &s, float &out)
{
    size_t i = 0, n = s.size();
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    const std::string body = s.substr(i);
    if (body == "inf") { out = neg ? -INFINITY : INFINITY; return true; }
    if (body == "NaN") { out = NAN; return true; }
    size_t j = i, nd = 0;
    while (j < n && isdigit((unsigned char)s[j])) { j++; nd++; }
    if (j < n && s[j] == '.') { j++; while (j < n && isdigit((unsigned char)s[j])) { j++; nd++; } }
    if (nd == 0) return false;
    if (j < n && (s[j] == 'e' || s[j] == 'E')) {
        j++;
        if (j < n && (s[j] == '+' || s[j] == '-')) j++;
        size_t ne = 0;
        while (j < n && isdigit((unsigned char)s[j])) { j++; ne++; }
        if (ne == 0) return false;
    }
    if (j != n) return false;
    out = strtof(s.c_str(), nullptr);
    return true;
}

static bool valid_utf8(const char *p, size_t n)
{
    const unsigned char *s = (const unsigned char *)p;
    size_t i = 0;
    while (i < n) {
        if (i + 8 <= n) {                       // ASCII fast path, 8 bytes at a time
            uint64_t v; memcpy(&v, s + i, 8);
            if (!(v & 0x8080808080808080ULL)) { i += 8; continue; }
        }
        unsigned char c = s[i];
        if (c < 0x80) { i++; continue; }
        int len; uint32_t cp, min;
        if ((c & 0xE0) == 0xC0) { len = 2; cp = c & 0x1F; min = 0x80; }
        else if ((c & 0xF0) == 0xE0) { len = 3; cp = c & 0x0F; min = 0x800; }
        else if ((c & 0xF8) == 0xF0) { len = 4; cp = c & 0x07; min = 0x10000; }
        else return false;
        if (i + len > n) return false;
        for (int k = 1; k < len; k++) { if ((s[i + k] & 0xC0) != 0x80) return false; cp = (cp << 6) | (s[i + k] & 0x3F); }
        if (cp < min || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
        i += len;
    }
    return true;
}

// Clinger's fast path in binary32: a decimal with < 2^24 mantissa and <= 10 fractional digits is
// float(m) / 10^f with both operands exact, so the single division rounds correctly -- the same
// value Rust's (correctly rounded) parser and strtof produce.  Anything else goes to parse_f32.
static bool parse_f32_fast(const char *p, size_t n, float &out)
{
    static const float P10[11] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f};
    uint32_t m = 0; size_t i = 0, nd = 0, frac = 0;
    for (; i < n && p[i] >= '0' && p[i] <= '9'; i++, nd++) { if (m > 1677721) return false; m = m * 10 + (uint32_t)(p[i] - '0'); }
    if (i < n && p[i] == '.') {
        for (i++; i < n && p[i] >= '0' && p[i] <= '9'; i++, nd++, frac++) { if (m > 1677721) return false; m = m * 10 + (uint32_t)(p[i] - '0'); }
    }
    if (i != n || nd == 0 || frac > 10 || m >= (1u << 24)) return false;
    out = (float)m / P10[frac];
    return true;
}

// title.split_whitespace()[2].split('=')[1].parse::<f32>().unwrap()   (main.rs:86-91 / :120-124)
static float header_depth(const char *t, size_t n)
{
    // str::split_whitespace(): Unicode White_Space (the line is already known to be valid UTF-8)
    auto ws_len = [&](size_t i) -> size_t {       // length of the white-space character at i, 0 if none
        const unsigned char c = (unsigned char)t[i];
        if (c < 0x80) return (c == ' ' || (c >= 9 && c <= 13)) ? 1 : 0;
        if (c == 0xC2 && i + 1 < n && ((unsigned char)t[i + 1] == 0x85 || (unsigned char)t[i + 1] == 0xA0)) return 2;
        if (i + 2 < n) {
            const unsigned char d = (unsigned char)t[i + 1], e = (unsigned char)t[i + 2];
            if (c == 0xE1 && d == 0x9A && e == 0x80) return 3;                                   // U+1680
            if (c == 0xE2 && d == 0x80 && ((e >= 0x80 && e <= 0x8A) || e == 0xA8 || e == 0xA9 || e == 0xAF)) return 3;   // U+2000-200A, 2028, 2029, 202F
            if (c == 0xE2 && d == 0x81 && e == 0x9F) return 3;                                   // U+205F
            if (c == 0xE3 && d == 0x80 && e == 0x80) return 3;                                   // U+3000
        }
        return 0;
    };
    size_t i = 0, ntok = 0, tb = 0, tl = 0;
    while (i < n && ntok < 3) {
        size_t l;
        while (i < n && (l = ws_len(i)) > 0) i += l;
        const size_t b = i;
        while (i < n && ws_len(i) == 0) i++;
        if (i > b) { ntok++; tb = b; tl = i - b; }
    }
    if (ntok < 3) rust_panic("index out of bounds: the len is " + std::to_string(ntok) + " but the index is 2");
    const char *f = t + tb;
    const char *e1 = (const char *)memchr(f, '=', tl);
    if (!e1) rust_panic("index out of bounds: the len is 1 but the index is 1");
    const char *vb = e1 + 1;
    const char *e2 = (const char *)memchr(vb, '=', (size_t)(f + tl - vb));
    const size_t vl = (size_t)((e2 ? e2 : f + tl) - vb);
    float v;
    if (parse_f32_fast(vb, vl, v)) return v;
    if (!parse_f32(std::string(vb, vl), v)) rust_panic("called `Result::unwrap()` on an `Err` value: ParseFloatError { kind: Invalid }");
    return v;
}

// ----------------------------------------------------------------- file IO
static bool has_gz_ext(const std::string &path)
{   // Path::extension() == Some("gz")  (helper.rs:19,34)
    size_t slash = path.rfind('/');
    std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    size_t dot = name.rfind('.');
    return dot != std::string::npos && dot != 0 && name.substr(dot) == ".gz";
}

// Input bytes: plain files are mapped (no copy), .gz files are inflated into `owned`.
struct Input { const char *p = nullptr; size_t n = 0; std::string owned; };

static void read_all(const std::string &path, std::string &data);
static void open_input(const std::string &path, Input &in)
{
    if (!has_gz_ext(path)) {
        int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) rust_panic("Cannot open file " + path + "!");
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
            close(fd);
            if (m != MAP_FAILED) { in.p = (const char *)m; in.n = (size_t)st.st_size; return; }
        } else close(fd);
    }
    read_all(path, in.owned);
    in.p = in.owned.data(); in.n = in.owned.size();
}

static void read_all(const std::string &path, std::string &data)
{
    if (has_gz_ext(path)) {
        FILE *probe = fopen(path.c_str(), "rb");
        if (!probe) rust_panic("Cannot open file " + path + "!");
        fclose(probe);
        gzFile g = gzopen(path.c_str(), "rb");
        if (!g) rust_panic("Cannot open file " + path + "!");
        gzbuffer(g, 128 * 1024);
        char buf[1 << 16]; int n;
        while ((n = gzread(g, buf, sizeof buf)) > 0) data.append(buf, (size_t)n);
        const bool bad = n < 0;
        gzclose(g);
        if (bad) rust_panic("called `Result::unwrap()` on an `Err` value: Custom { kind: InvalidInput, error: \"corrupt deflate stream\" }");
        return;
    }
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) rust_panic("Cannot open file " + path + "!");
    struct stat st;
    size_t have = 0;
    if (fstat(fileno(f), &st) == 0 && st.st_size > 0) {      // regular file: one allocation, one read
        data.resize((size_t)st.st_size);
        have = fread(&data[0], 1, data.size(), f);
        data.resize(have);
    }
    char buf[1 << 16]; size_t n;                              // pipes / files that grew
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.append(buf, n);
    fclose(f);
}

struct Writer {
    bool gz = false; gzFile g = nullptr; FILE *f = nullptr; std::string buf;
    void open(const std::string &path)
    {
        gz = has_gz_ext(path);
        if (gz) { g = gzopen(path.c_str(), "wb6"); if (!g) rust_panic("Cannot open file " + path); }   // Compression::default() = level 6
        else { f = fopen(path.c_str(), "wb"); if (!f) rust_panic("Cannot open file " + path); }
        buf.reserve((1u << 20) + 65536);
    }
    void drain() { if (buf.empty()) return; if (gz) gzwrite(g, buf.data(), (unsigned)buf.size()); else fwrite(buf.data(), 1, buf.size(), f); buf.clear(); }
    void line(const char *p, size_t n) { buf.append(p, n); buf.push_back('\n'); if (buf.size() >= (1u << 20)) drain(); }
    void close() { drain(); if (gz && g) gzclose(g); if (f) fclose(f); g = nullptr; f = nullptr; }
};

struct Line { const char *p; size_t n; };
// BufRead::lines(): split at '\n', drop one trailing '\r', final line may lack '\n', empty trailing piece not yielded
static void split_lines(const Input &data, std::vector<Line> &lines)
{
    const char *p = data.p, *end = p + data.n;
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl : end;
        size_t n = (size_t)(le - p);
        if (n && p[n - 1] == '\r') n--;
        lines.push_back(Line{p, n});
        if (!nl) break;
        p = nl + 1;
    }
}

// ------------------------------------------------------------ contig filter
static int contig_filter_main(int argc, char **argv)
{
    std::string v_l, v_d, v_i, v_o, v_m;
    bool has_l = false, has_d = false, has_i = false, has_o = false, has_m = false;
    for (int a = 1; a < argc; a++) {
        std::string arg = argv[a];
        if (arg == "-h" || arg == "--help") { print_help(); return 0; }
        if (arg == "-V" || arg == "--version") { puts("Length filter 0.1"); return 0; }
        if (arg.size() < 2 || arg[0] != '-' || arg[1] == '-')
            clap_error("Found argument '" + arg + "' which wasn't expected, or isn't valid in this context");
        const char o = arg[1];
        if (o != 'l' && o != 'd' && o != 'i' && o != 'o' && o != 'm')
            clap_error("Found argument '-" + std::string(1, o) + "' which wasn't expected, or isn't valid in this context");
        std::string val;
        if (arg.size() > 2) { val = arg.substr(2); if (val[0] == '=') val = val.substr(1); }
        else {
            if (a + 1 >= argc) clap_error("The argument '-" + std::string(1, o) + " <" + (o == 'i' || o == 'o' ? "PATH" : o == 'l' ? "INT,INT" : "INT") + ">' requires a value but none was supplied");
            val = argv[++a];
            if (!val.empty() && val[0] == '-' && val.size() > 1)
                clap_error("Found argument '" + val + "' which wasn't expected, or isn't valid in this context");
        }
        bool *has = o == 'l' ? &has_l : o == 'd' ? &has_d : o == 'i' ? &has_i : o == 'o' ? &has_o : &has_m;
        std::string *dst = o == 'l' ? &v_l : o == 'd' ? &v_d : o == 'i' ? &v_i : o == 'o' ? &v_o : &v_m;
        if (*has) clap_error("The argument '-" + std::string(1, o) + "' was provided more than once, but cannot be used multiple times");
        *has = true; *dst = val;
    }
    if (has_d && has_m) clap_error("The argument '-d <INT>' cannot be used with '-m <INT>'");
    if (!has_i || !has_l || !has_o) {
        std::string miss;
        if (!has_i) miss += "\n    -i <PATH>";
        if (!has_l) miss += "\n    -l <INT,INT>";
        if (!has_o) miss += "\n    -o <PATH>";
        clap_error("The following required arguments were not provided:" + miss);
    }

    // main.rs:57-67
    std::vector<uint64_t> lengths;
    {
        size_t b = 0;
        for (;;) {
            size_t c = v_l.find(',', b);
            std::string piece = v_l.substr(b, c == std::string::npos ? std::string::npos : c - b);
            uint64_t v;
            if (!piece.empty()) {                // clap's delimiter split drops empty pieces (golden X37)
                if (!parse_usize(piece, v)) rust_panic("called `Result::unwrap()` on an `Err` value: ParseIntError { kind: InvalidDigit }");
                lengths.push_back(v);
            }
            if (c == std::string::npos) break;
            b = c + 1;
        }
    }
    if (lengths.size() != 2) { puts("Input length string not valid, please input INT,INT."); }
    if (lengths.size() < 2) rust_panic("index out of bounds: the len is " + std::to_string(lengths.size()) + " but the index is " + std::to_string(lengths.size()));
    const uint64_t min = lengths[0], max = lengths[1];

    Input data; open_input(v_i, data);           // main.rs:69
    static Writer out; out.open(v_o);            // main.rs:70
    g_flush_on_panic = [] { out.close(); };
    uint64_t count = 0;
    std::vector<Line> lines;

    if (!has_m) {
        // main.rs:74-105 -- pairs of lines are taken straight off the buffer (lines().tuples())
        if (!has_d) rust_panic("called `Option::unwrap()` on a `None` value");
        int32_t depth;
        if (!parse_i32(v_d, depth)) rust_panic("called `Result::unwrap()` on an `Err` value: ParseIntError { kind: InvalidDigit }");
        const char *p = data.p, *end = p + data.n;
        auto next_line = [&](Line &l) -> bool {      // BufRead::lines(): split at LF, drop one trailing CR
            if (p >= end) return false;
            const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
            const char *le = nl ? nl : end;
            size_t n = (size_t)(le - p);
            if (n && p[n - 1] == '\r') n--;
            l = Line{p, n};
            p = nl ? nl + 1 : end;
            return true;
        };
        Line t, s;
        while (next_line(t) && next_line(s)) {
            if (!valid_utf8(t.p, t.n) || !valid_utf8(s.p, s.n)) rust_panic("called `Result::unwrap()` on an `Err` value: Custom { kind: InvalidData, error: \"stream did not contain valid UTF-8\" }");
            if (t.n == 0 || t.p[0] != '>') continue;
            if (depth != 0) {
                const float seq_depth = header_depth(t.p, t.n);
                if ((float)depth > seq_depth) continue;
            }
            const uint64_t length = (uint64_t)s.n - 1;            // wraps for an empty sequence, as the release binary does
            if (length < min || length > max) continue;
            out.line(t.p, t.n); out.line(s.p, s.n);
            count++;
        }
    } else {
        // main.rs:106-131
        split_lines(data, lines);
        uint64_t max_count;
        if (!parse_usize(v_m, max_count)) rust_panic("called `Result::unwrap()` on an `Err` value: ParseIntError { kind: InvalidDigit }");
        for (const Line &l : lines)
            if (!valid_utf8(l.p, l.n)) rust_panic("called `Result::unwrap()` on an `Err` value: Custom { kind: InvalidData, error: \"stream did not contain valid UTF-8\" }");
        std::vector<std::pair<Line, Line>> seqs;
        for (size_t i = 0; i + 1 < lines.size(); i += 2)
            if (lines[i + 1].n <= max && lines[i + 1].n >= min) seqs.emplace_back(lines[i], lines[i + 1]);
        // sort_by_cached_key with a unit key: stable no-op, but the key closure still
        // runs (and can panic) for every element when there are at least two
        if (seqs.size() >= 2) for (auto &p : seqs) (void)header_depth(p.first.p, p.first.n);
        for (size_t j = seqs.size(); j-- > 0 && count < max_count;) {
            out.line(seqs[j].first.p, seqs[j].first.n); out.line(seqs[j].second.p, seqs[j].second.n);
            count++;
        }
    }
    g_flush_on_panic = nullptr;
    out.close();
    printf("%llu\n", (unsigned long long)count);
    return 0;
}

// ---------------------------------------------------------------- bait mode
static std::string exe_dir()
{
    char buf[PATH_MAX]; ssize_t n = readlink("/proc/self/exe", buf, sizeof buf - 1);
    if (n <= 0) return ".";
    buf[n] = 0;
    std::string p(buf); size_t s = p.rfind('/');
    return s == std::string::npos ? "." : p.substr(0, s);
}

// what the command line asks for (checked: one kind of report at most)
struct BaitArgs {
    std::string bait, fq1, fq2, out1, out2, pair = "either", libpath, report, group_report, group_sep, depth_report, depth_profile, place_report, base_depth_file, pileup_file, consensus_file,
                variants_file, score_report, indels_file, gapped_file, insertions_file, extended_file, extension_report;
    unsigned min_depth = 1, thr = 1, max_permille = 1000, band = 0, extend = 0;          // extend: --extend, the columns an end may grow by
    bool aligned = false;                      // --band: the placed reads are aligned inside the band before they are scored and cut
    int keep = MF_KEEP_PASSING;                // --write: which mates the verifying call writes
    int group_field = -1, k = 0, devices = 1, gcode = 5; bool protein = false;
    std::vector<int> device_list;              // --device-list 2,3: these devices instead of 0 .. N - 1
    std::vector<std::pair<std::string, std::string>> options;      // --option pass=serial: how a filter pass is run (mf_set_option)
    bool grouped = false, depth = false, placed = false, piled = false;          // which report (grouped: `report` holds --group-report's file)
    bool verified = false;                     // --score-report, --max-mismatch or --write accepted|placed: the placed reads are scored (and cut) first
};

// what the library's call gave: the arrays the report files are written from
struct BaitResult {
    uint64_t kept = 0, total = 0, unplaced[2] = {0, 0};
    std::vector<std::string> names;          // of the records, or the groups
    std::vector<uint64_t> starts, counts;
    std::vector<uint32_t> profile;          // k-mer depth or base depth
    std::vector<mf_depth_record_t> depth_recs;
    std::vector<mf_place_record_t> place_recs;
    std::vector<mf_pileup_t> pile;
    std::vector<uint8_t> consensus, letters;
    std::vector<mf_score_record_t> score_recs;
    std::vector<mf_align_record_t> align_recs;          // with --band, in place of score_recs
    std::vector<mf_indel_t> indels;
    std::vector<mf_pileup_t> ins_pile;          // with --gapped-consensus or --insertions: 2 * band entries a position
    std::vector<uint8_t> gapped; std::vector<uint64_t> gapped_starts;
    std::vector<mf_pileup_t> ext_pile;          // with --extend: 2 * extend entries a record
    std::vector<uint8_t> extended; std::vector<uint64_t> extended_starts;
};

// 0, or the exit code of a command line that cannot be run
static int parse_bait_args(int argc, char **argv, BaitArgs &A)
{
    bool have_min_depth = false, have_sep = false, have_max_mismatch = false, have_band = false;
    for (int a = 2; a < argc; a++) {
        std::string o = argv[a];
        auto need = [&](const char *name) -> std::string {
            if (a + 1 >= argc) { fprintf(stderr, "error: %s requires a value\n", name); exit(1); }
            return argv[++a];
        };
        if (o == "--bait") A.bait = need("--bait");
        else if (o == "--fq1") A.fq1 = need("--fq1");
        else if (o == "--fq2") A.fq2 = need("--fq2");
        else if (o == "--out1") A.out1 = need("--out1");
        else if (o == "--out2") A.out2 = need("--out2");
        else if (o == "--pair") A.pair = need("--pair");
        else if (o == "--lib") A.libpath = need("--lib");
        else if (o == "--report") A.report = need("--report");
        else if (o == "--group-report") A.group_report = need("--group-report");
        else if (o == "--depth-report") A.depth_report = need("--depth-report");
        else if (o == "--depth-profile") A.depth_profile = need("--depth-profile");
        else if (o == "--place-report") A.place_report = need("--place-report");
        else if (o == "--base-depth") A.base_depth_file = need("--base-depth");
        else if (o == "--pileup") A.pileup_file = need("--pileup");
        else if (o == "--consensus") A.consensus_file = need("--consensus");
        else if (o == "--variants") A.variants_file = need("--variants");
        else if (o == "--min-depth") {
            const std::string v = need("--min-depth"); char *end = nullptr; const unsigned long x = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] == '-' || x < 1 || x > 0xFFFFFFFFul) { fprintf(stderr, "error: --min-depth wants a depth from 1\n"); return 1; }
            A.min_depth = (unsigned)x; have_min_depth = true;
        }
        else if (o == "--score-report") A.score_report = need("--score-report");
        else if (o == "--max-mismatch") {
            const std::string v = need("--max-mismatch"); char *end = nullptr; const unsigned long x = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] < '0' || v[0] > '9' || x > 1000) { fprintf(stderr, "error: --max-mismatch wants mismatches per thousand compared bases, from 0 to 1000\n"); return 1; }
            A.max_permille = (unsigned)x; have_max_mismatch = true;
        }
        else if (o == "--band") {
            const std::string v = need("--band"); char *end = nullptr; const unsigned long x = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] < '0' || v[0] > '9' || x > 31) { fprintf(stderr, "error: --band wants a number of diagonals on either side of the placement's, from 0 to 31 (and below k)\n"); return 1; }
            A.band = (unsigned)x; have_band = true;
        }
        else if (o == "--indels") A.indels_file = need("--indels");
        else if (o == "--gapped-consensus") A.gapped_file = need("--gapped-consensus");
        else if (o == "--insertions") A.insertions_file = need("--insertions");
        else if (o == "--extend") {
            const std::string v = need("--extend"); char *end = nullptr; const unsigned long x = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] < '0' || v[0] > '9' || x < 1 || x > MF_EXTEND_MAX) { fprintf(stderr, "error: --extend wants the columns a record end may grow by, from 1 to %d\n", MF_EXTEND_MAX); return 1; }
            A.extend = (unsigned)x;
        }
        else if (o == "--extended-consensus") A.extended_file = need("--extended-consensus");
        else if (o == "--extension-report") A.extension_report = need("--extension-report");
        else if (o == "--write") {
            const std::string v = need("--write");
            if (v == "passing") A.keep = MF_KEEP_PASSING; else if (v == "accepted") A.keep = MF_KEEP_ACCEPTED; else if (v == "placed") A.keep = MF_KEEP_PLACED;
            else { fprintf(stderr, "error: --write wants passing, accepted or placed\n"); return 1; }
        }
        else if (o == "--group-field") {
            const std::string v = need("--group-field"); char *end = nullptr; const long x = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || x < 1 || x > INT_MAX) { fprintf(stderr, "error: --group-field wants a field number from 1\n"); return 1; }
            A.group_field = (int)x;
        }
        else if (o == "--group-sep") { A.group_sep = need("--group-sep"); have_sep = true; if (A.group_sep.empty()) { fprintf(stderr, "error: --group-sep wants a separator\n"); return 1; } }
        else if (o == "-k" || o == "--kmer") A.k = atoi(need("-k").c_str());
        else if (o == "-t" || o == "--threshold") A.thr = (unsigned)strtoul(need("-t").c_str(), nullptr, 10);
        else if (o == "--devices") A.devices = atoi(need("--devices").c_str());
        else if (o == "--device-list") {
            const std::string v = need("--device-list");
            for (size_t i = 0; i < v.size();) { size_t j = v.find(',', i); if (j == std::string::npos) j = v.size(); if (j > i) A.device_list.push_back(atoi(v.substr(i, j - i).c_str())); i = j + 1; }
            if (A.device_list.empty()) { fprintf(stderr, "error: --device-list wants device numbers separated by commas\n"); return 1; }
        }
        else if (o == "--option") {
            const std::string v = need("--option"); const size_t eq = v.find('=');
            if (eq == std::string::npos || eq == 0) { fprintf(stderr, "error: --option wants name=value\n"); return 1; }
            A.options.emplace_back(v.substr(0, eq), v.substr(eq + 1));
        }
        else if (o == "--protein") A.protein = true;                       // --bait is a protein FASTA (e.g. profile/MT_database/<clade>.fa)
        else if (o == "--code" || o == "--genetic-code") A.gcode = atoi(need("--code").c_str());
        else { fprintf(stderr, "error: unknown option '%s' for fastfilter bait\n", o.c_str()); return 1; }
    }
    if (A.bait.empty() || A.fq1.empty() || A.out1.empty() || (A.fq2.empty() != A.out2.empty()) || (A.pair != "either" && A.pair != "both")) {
        fputs("usage: fastfilter bait --bait BAIT.fa [-k 31] [-t 1] --fq1 R1.fq [--fq2 R2.fq] --out1 O1.fq [--out2 O2.fq]"
              " [--pair either|both] [--devices N | --device-list D0,D1,..] [--option name=value ..]\n"
              "       [--report FILE | --group-report FILE [--group-field N] [--group-sep C] | --depth-report FILE [--depth-profile FILE]\n"
              "        | --place-report FILE [--base-depth FILE] | [--pileup FILE] [--consensus FILE] [--variants FILE] [--min-depth N]]\n"
              "       [--score-report FILE] [--max-mismatch PERMILLE]   (with or without the placement or the pile-up reports)\n"
              "       [--band W [--indels FILE] [--gapped-consensus FILE] [--insertions FILE]\n"
              "        [--extend E [--extended-consensus FILE] [--extension-report FILE]]]   (wherever --max-mismatch may go: the placed reads are aligned inside 2 W + 1 diagonals, indels cost one edit a base)\n"
              "       [--write passing|accepted|placed]   (which mates are written: all that pass, not those the cut rejects, only placed and accepted ones)\n"
              "       fastfilter bait --protein --bait PROTEINS.fa [--code 5] [-k 9] ...   (six-frame peptide k-mers)\n", stderr);
        return 1;
    }
    if (A.protein && !A.report.empty()) { fprintf(stderr, "error: --report needs a nucleotide bait (it cannot be combined with --protein)\n"); return 1; }
    if (!A.report.empty() && !A.group_report.empty()) { fprintf(stderr, "error: --report and --group-report cannot be combined\n"); return 1; }
    const bool depth = A.depth = !A.depth_report.empty() || !A.depth_profile.empty();
    if (depth && (!A.report.empty() || !A.group_report.empty())) { fprintf(stderr, "error: --depth-report / --depth-profile cannot be combined with --report or --group-report\n"); return 1; }
    const bool placed = A.placed = !A.place_report.empty() || !A.base_depth_file.empty();
    if (placed && (depth || A.protein || !A.report.empty() || !A.group_report.empty())) {
        fprintf(stderr, "error: --place-report / --base-depth need a nucleotide bait and cannot be combined with --report, --group-report, --depth-report, --depth-profile or --protein\n");
        return 1;
    }
    const bool piled = A.piled = !A.pileup_file.empty() || !A.consensus_file.empty() || !A.variants_file.empty();
    if (piled && (placed || depth || A.protein || !A.report.empty() || !A.group_report.empty())) {
        fprintf(stderr, "error: --pileup / --consensus / --variants need a nucleotide bait and cannot be combined with --report, --group-report, --depth-report, --depth-profile, --place-report, --base-depth or --protein\n");
        return 1;
    }
    const bool gapped = !A.gapped_file.empty() || !A.insertions_file.empty();
    if (gapped && !have_band) { fprintf(stderr, "error: --gapped-consensus and --insertions need --band\n"); return 1; }
    if ((!A.extended_file.empty() || !A.extension_report.empty()) && !A.extend) { fprintf(stderr, "error: --extended-consensus and --extension-report need --extend\n"); return 1; }
    if (A.extend && !have_band) { fprintf(stderr, "error: --extend needs --band (--band 0 is fine)\n"); return 1; }
    if (have_min_depth && !piled && A.gapped_file.empty() && A.extended_file.empty()) { fprintf(stderr, "error: --min-depth needs --pileup, --consensus or --variants\n"); return 1; }
    const bool keeping = A.keep != MF_KEEP_PASSING;
    if (have_max_mismatch && !placed && !piled && A.score_report.empty() && !keeping && !A.extend) {
        fprintf(stderr, "error: --max-mismatch needs --place-report, --base-depth, --pileup, --consensus, --variants, --score-report, --extend or --write accepted|placed\n");
        return 1;
    }
    if (have_band && !placed && !piled && A.score_report.empty() && !keeping && A.indels_file.empty() && !gapped && !A.extend) {
        fprintf(stderr, "error: --band needs --place-report, --base-depth, --pileup, --consensus, --variants, --score-report, --indels or --write accepted|placed\n");
        return 1;
    }
    if (!A.indels_file.empty() && !have_band) { fprintf(stderr, "error: --indels needs --band\n"); return 1; }
    if (have_band && (depth || A.protein || !A.report.empty() || !A.group_report.empty())) {
        fprintf(stderr, "error: --band needs a nucleotide bait and cannot be combined with --report, --group-report, --depth-report, --depth-profile or --protein\n");
        return 1;
    }
    if (keeping && (depth || A.protein || !A.report.empty() || !A.group_report.empty())) {
        fprintf(stderr, "error: --write accepted|placed needs a nucleotide bait and cannot be combined with --report, --group-report, --depth-report, --depth-profile or --protein\n");
        return 1;
    }
    if (!A.score_report.empty() && (depth || A.protein || !A.report.empty() || !A.group_report.empty())) {
        fprintf(stderr, "error: --score-report needs a nucleotide bait and cannot be combined with --report, --group-report, --depth-report, --depth-profile or --protein\n");
        return 1;
    }
    A.verified = have_max_mismatch || !A.score_report.empty() || keeping || have_band;
    A.aligned = have_band;
    if (A.group_report.empty() && (A.group_field >= 0 || have_sep)) { fprintf(stderr, "error: --group-field and --group-sep need --group-report\n"); return 1; }
    if (!have_sep) A.group_sep = "_";
    if (A.k == 0) A.k = A.protein ? 9 : 31;
    if (have_band && (int)A.band >= A.k) { fprintf(stderr, "error: --band stays below k (%d)\n", A.k); return 1; }
    if (A.libpath.empty()) { const char *e = getenv("MITOFILTER_LIB"); if (e && *e) A.libpath = e; }          // (as the Python wrapper and filter_v2 do)
    if (A.libpath.empty()) A.libpath = exe_dir() + "/../libmitofilter_hip.so";
    A.grouped = !A.group_report.empty();
    if (A.grouped) A.report = A.group_report;
    return 0;
}

// the names of a set's records or groups (count and name_of: the library's pair of calls for either)
static int fetch_names(const mf_kmerset *ks, decltype(&mf_kmerset_record_count) count, decltype(&mf_kmerset_record_name) name_of, std::vector<std::string> &names)
{
    uint64_t n = 0;
    int rc = count(ks, &n);
    for (uint64_t i = 0; rc == MF_OK && i < n; i++) {
        size_t need = 0;
        (void)name_of(ks, i, nullptr, 0, &need);
        std::vector<char> buf(need ? need : 1);
        rc = name_of(ks, i, buf.data(), buf.size(), nullptr);
        names.emplace_back(buf.data());
    }
    return rc;
}

static int fetch_starts(const mf_kmerset *ks, decltype(&mf_kmerset_record_starts) record_starts, size_t n_rec, std::vector<uint64_t> &starts)
{
    starts.assign(n_rec + 1, 0);
    return record_starts(ks, starts.data(), starts.size(), nullptr);
}

// what mf_filter_fastq_files does with a device count: 0 .. N - 1, at most the devices there are
static void default_devices(decltype(&mf_device_count) device_count, int devices, std::vector<int> &list)
{
    if (!list.empty()) return;
    const int have = device_count();
    for (int i = 0; i < std::min(std::max(devices, 1), std::max(have, 1)); i++) list.push_back(i);
}

// Loads the library, builds the bait set and runs the file-level call of the report that is asked for.  0 with *ks and *free_set for
// the caller to end with, or the exit code (the set is freed).
static int bait_run(const BaitArgs &A, BaitResult &R, mf_kmerset **ks_out, decltype(&mf_kmerset_free) *free_set)
{
    void *h = dlopen(A.libpath.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "error: cannot load %s: %s (the bait filter has no CPU fallback)\n", A.libpath.c_str(), dlerror()); return 2; }
    mf_kmerset *ks = nullptr;
    // a symbol of the library, looked up where it is needed; without it the set (if it is built) is freed and the exit code is 2
#define SYM(name) auto p_##name = (decltype(&name))dlsym(h, #name); if (!p_##name) { fprintf(stderr, "error: %s lacks symbol %s\n", A.libpath.c_str(), #name); if (ks) (*free_set)(ks); return 2; }
    SYM(mf_abi_version) SYM(mf_last_error) SYM(mf_kmerset_build_from_fasta) SYM(mf_kmerset_build_protein_from_fasta)
    SYM(mf_filter_fastq_files) SYM(mf_filter_fastq_files_on) SYM(mf_kmerset_free) SYM(mf_set_option)
    *free_set = p_mf_kmerset_free;
    if (p_mf_abi_version() != MF_ABI_VERSION) { fprintf(stderr, "error: ABI version mismatch\n"); return 2; }
    (void)p_mf_set_option("expect_files", "1"); (void)p_mf_set_option("short_lived", "1");          // (the file-level call's set-up starts beside the bait set's build)
    for (auto &kv : A.options) if (p_mf_set_option(kv.first.c_str(), kv.second.c_str()) != MF_OK) { fprintf(stderr, "error: %s\n", p_mf_last_error()); return 1; }
    mf::cold_mark("library loaded");
    std::vector<int> device_list = A.device_list;
    const int dev0 = device_list.empty() ? 0 : device_list[0];
    const int brc = A.protein ? p_mf_kmerset_build_protein_from_fasta(A.bait.c_str(), A.k, A.gcode, dev0, &ks)
                              : p_mf_kmerset_build_from_fasta(A.bait.c_str(), A.k, dev0, &ks);
    if (brc != MF_OK) { fprintf(stderr, "error: %s\n", p_mf_last_error()); return 3; }
    mf::cold_mark("bait set built");
    setenv("MF_DEVPOOL_GB", "4096", 0);          // (a process that ends with the call gives no device memory back in between: the runtime frees it all at once)
    // the files and the pair rule of every call; `files`: a call on the device list, with its own outputs in the middle
    const char *fq1 = A.fq1.c_str(), *fq2 = A.fq2.empty() ? nullptr : A.fq2.c_str(), *out1 = A.out1.c_str(), *out2 = A.out2.empty() ? nullptr : A.out2.c_str();
    const int pair_mode = A.pair == "both" ? MF_PAIR_BOTH : MF_PAIR_EITHER;
    auto files = [&](auto call, auto... outs) { return call(ks, fq1, fq2, out1, out2, A.thr, pair_mode, device_list.data(), (int)device_list.size(), outs..., &R.kept, &R.total); };
    int rc;
    if (A.piled || A.placed || A.depth || A.verified) {
        SYM(mf_device_count) SYM(mf_kmerset_record_starts)
        if (A.depth) {          // (the identity grouping: the records' own names, protein sets included)
            SYM(mf_kmerset_group_count) SYM(mf_kmerset_group_name)
            rc = fetch_names(ks, p_mf_kmerset_group_count, p_mf_kmerset_group_name, R.names);
        } else {
            SYM(mf_kmerset_record_count) SYM(mf_kmerset_record_name)
            rc = fetch_names(ks, p_mf_kmerset_record_count, p_mf_kmerset_record_name, R.names);
        }
        if (rc == MF_OK) rc = fetch_starts(ks, p_mf_kmerset_record_starts, R.names.size(), R.starts);
        if (rc == MF_OK) default_devices(p_mf_device_count, A.devices, device_list);
        const size_t positions = rc == MF_OK ? (size_t)std::max<uint64_t>(R.starts.back(), 1) : 1, n_rec = std::max<size_t>(R.names.size(), 1);
        if (A.verified) {          // the placed reads scored and cut; then what the family asks for, from the accepted ones
            SYM(mf_kmerset_bait_letters) SYM(mf_filter_fastq_files_verified_keep)
            const bool with_depth = A.placed || !A.indels_file.empty() || !A.insertions_file.empty();          // (the indel tables are written beside the base depth)
            R.score_recs.assign(n_rec, mf_score_record_t{});
            if (A.piled) { R.pile.assign(positions, mf_pileup_t{}); R.consensus.assign(positions, 0); R.letters.assign(positions, 0); }
            if (with_depth) { R.profile.assign(positions, 0); R.place_recs.assign(n_rec, mf_place_record_t{}); }
            if (rc == MF_OK && A.piled) rc = p_mf_kmerset_bait_letters(ks, R.letters.data(), R.letters.size(), nullptr);
            if (rc == MF_OK && A.aligned && A.extend) {          // ... with the records' ends extended (and the gapped outputs where they are asked for)
                SYM(mf_filter_fastq_files_extended)
                const size_t span = 2 * (size_t)A.band, E = A.extend;
                const bool gap = !A.gapped_file.empty() || !A.insertions_file.empty();
                R.align_recs.assign(n_rec, mf_align_record_t{}); R.indels.assign(positions, mf_indel_t{});
                if (gap) { R.ins_pile.assign(std::max<size_t>(positions * span, 1), mf_pileup_t{}); R.gapped.assign(positions * (1 + span), 0); R.gapped_starts.assign(n_rec + 1, 0); }
                R.ext_pile.assign(n_rec * 2 * E, mf_pileup_t{}); R.extended.assign(positions * (1 + span) + 2 * n_rec * E, 0); R.extended_starts.assign(n_rec + 1, 0);
                rc = files(p_mf_filter_fastq_files_extended, A.min_depth, A.max_permille, A.keep, A.band, A.extend, with_depth ? R.profile.data() : nullptr,
                           with_depth ? R.place_recs.data() : nullptr, A.piled ? R.pile.data() : nullptr, A.piled ? R.consensus.data() : nullptr, (mf_pileup_record_t *)nullptr,
                           R.indels.data(), R.align_recs.data(), gap && span ? R.ins_pile.data() : nullptr, gap ? R.gapped.data() : nullptr,
                           gap ? R.gapped_starts.data() : nullptr, (mf_gapped_record_t *)nullptr, R.ext_pile.data(), R.extended.data(), R.extended_starts.data(),
                           (mf_extend_record_t *)nullptr, R.unplaced);
            } else if (rc == MF_OK && A.aligned && (!A.gapped_file.empty() || !A.insertions_file.empty())) {          // ... and with the gapped consensus
                SYM(mf_filter_fastq_files_gapped)
                const size_t span = 2 * (size_t)A.band;
                R.align_recs.assign(n_rec, mf_align_record_t{}); R.indels.assign(positions, mf_indel_t{});
                R.ins_pile.assign(std::max<size_t>(positions * span, 1), mf_pileup_t{}); R.gapped.assign(positions * (1 + span), 0); R.gapped_starts.assign(n_rec + 1, 0);
                rc = files(p_mf_filter_fastq_files_gapped, A.min_depth, A.max_permille, A.keep, A.band, with_depth ? R.profile.data() : nullptr, with_depth ? R.place_recs.data() : nullptr,
                           A.piled ? R.pile.data() : nullptr, A.piled ? R.consensus.data() : nullptr, (mf_pileup_record_t *)nullptr, R.indels.data(), R.align_recs.data(),
                           span ? R.ins_pile.data() : nullptr, R.gapped.data(), R.gapped_starts.data(), (mf_gapped_record_t *)nullptr, R.unplaced);
            } else if (rc == MF_OK && A.aligned) {          // the same behind the banded alignment
                SYM(mf_filter_fastq_files_aligned)
                R.align_recs.assign(n_rec, mf_align_record_t{}); R.indels.assign(positions, mf_indel_t{});
                rc = files(p_mf_filter_fastq_files_aligned, A.min_depth, A.max_permille, A.keep, A.band, with_depth ? R.profile.data() : nullptr, with_depth ? R.place_recs.data() : nullptr,
                           A.piled ? R.pile.data() : nullptr, A.piled ? R.consensus.data() : nullptr, (mf_pileup_record_t *)nullptr, R.indels.data(), R.align_recs.data(), R.unplaced);
            } else if (rc == MF_OK)
                rc = files(p_mf_filter_fastq_files_verified_keep, A.min_depth, A.max_permille, A.keep, A.placed ? R.profile.data() : nullptr, A.placed ? R.place_recs.data() : nullptr,
                           A.piled ? R.pile.data() : nullptr, A.piled ? R.consensus.data() : nullptr, (mf_pileup_record_t *)nullptr, R.score_recs.data(), R.unplaced);
        } else if (A.piled) {
            SYM(mf_kmerset_bait_letters) SYM(mf_filter_fastq_files_pileup)
            R.pile.assign(positions, mf_pileup_t{}); R.consensus.assign(positions, 0); R.letters.assign(positions, 0);
            if (rc == MF_OK) rc = p_mf_kmerset_bait_letters(ks, R.letters.data(), R.letters.size(), nullptr);
            if (rc == MF_OK) rc = files(p_mf_filter_fastq_files_pileup, A.min_depth, R.pile.data(), R.consensus.data(), (mf_pileup_record_t *)nullptr, R.unplaced);
        } else if (A.placed) {
            SYM(mf_filter_fastq_files_placed)
            R.profile.assign(positions, 0);          // (the base depth: the report's max column needs it too)
            R.place_recs.assign(n_rec, mf_place_record_t{});
            if (rc == MF_OK) rc = files(p_mf_filter_fastq_files_placed, R.profile.data(), R.place_recs.data(), R.unplaced);
        } else {
            SYM(mf_filter_fastq_files_depth)
            R.profile.assign(positions, 0);
            R.depth_recs.assign(n_rec, mf_depth_record_t{});
            if (rc == MF_OK) rc = files(p_mf_filter_fastq_files_depth, R.profile.data(), R.depth_recs.data());
        }
    } else if (!A.report.empty()) {
        SYM(mf_device_count) SYM(mf_kmerset_record_count) SYM(mf_kmerset_record_name) SYM(mf_filter_fastq_files_by_record)
        SYM(mf_kmerset_group_records) SYM(mf_kmerset_group_count) SYM(mf_kmerset_group_name) SYM(mf_filter_fastq_files_by_group)
        rc = A.grouped ? p_mf_kmerset_group_records(ks, A.group_field > 0 ? A.group_sep.c_str() : nullptr, A.group_field > 0 ? A.group_field : 0) : MF_OK;
        if (rc == MF_OK) rc = A.grouped ? fetch_names(ks, p_mf_kmerset_group_count, p_mf_kmerset_group_name, R.names)
                                        : fetch_names(ks, p_mf_kmerset_record_count, p_mf_kmerset_record_name, R.names);
        if (rc == MF_OK) default_devices(p_mf_device_count, A.devices, device_list);
        R.counts.assign(R.names.size() + 2, 0);
        if (rc == MF_OK) rc = files(A.grouped ? p_mf_filter_fastq_files_by_group : p_mf_filter_fastq_files_by_record, R.counts.data());
    } else rc = device_list.empty() ? p_mf_filter_fastq_files(ks, fq1, fq2, out1, out2, A.thr, pair_mode, A.devices, &R.kept, &R.total)
                                    : files(p_mf_filter_fastq_files_on);
#undef SYM
    if (rc != MF_OK) { fprintf(stderr, "error: %s\n", p_mf_last_error()); p_mf_kmerset_free(ks); return 3; }
    *ks_out = ks;
    return 0;
}

// one report file: open, write (mf_report_text.h), close; false with the message when any of that fails
template <class Write> static bool write_file(const std::string &path, const char *what, Write write)
{
    if (path.empty()) return true;
    FILE *f = fopen(path.c_str(), "w");
    bool ok = write(f);
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) fprintf(stderr, "error: cannot write the %s %s\n", what, path.c_str());
    return ok;
}

static bool write_reports(const BaitArgs &A, const BaitResult &R)
{
    using namespace mf_text;
    return write_file(A.report, "report", [&](FILE *f) { return write_reads(f, A.grouped, R.names, R.counts.data()); })
        && write_file(A.depth_report, "depth report", [&](FILE *f) { return write_depth_report(f, R.names, R.starts, R.depth_recs.data()); })
        && write_file(A.depth_profile, "depth profile", [&](FILE *f) { return write_depth_profile(f, R.names, R.starts, R.profile.data()); })
        && write_file(A.place_report, "placement report", [&](FILE *f) { return write_place_report(f, R.names, R.starts, R.place_recs.data(), R.profile.data(), R.unplaced[0]); })
        && write_file(A.base_depth_file, "base depth", [&](FILE *f) { return write_base_depth(f, R.names, R.starts, R.profile.data()); })
        && write_file(A.pileup_file, "pile-up", [&](FILE *f) { return write_pileup(f, R.names, R.starts, R.letters.data(), R.pile.data()); })
        && write_file(A.consensus_file, "consensus", [&](FILE *f) { return write_consensus(f, R.names, R.starts, R.consensus.data()); })
        && write_file(A.variants_file, "variants", [&](FILE *f) { return write_variants(f, R.names, R.starts, R.letters.data(), R.pile.data(), R.consensus.data()); })
        && write_file(A.score_report, "score report", [&](FILE *f) { return A.aligned ? write_align_report(f, R.names, R.starts, R.align_recs.data())
                                                                                      : write_score_report(f, R.names, R.starts, R.score_recs.data()); })
        && write_file(A.indels_file, "indel table", [&](FILE *f) { return write_indels(f, R.names, R.starts, R.profile.data(), R.indels.data()); })
        && write_file(A.gapped_file, "gapped consensus", [&](FILE *f) { return write_gapped_consensus(f, R.names, R.gapped_starts.data(), R.gapped.data()); })
        && write_file(A.insertions_file, "insertion table", [&](FILE *f) { return write_insertions(f, R.names, R.starts, R.profile.data(), R.ins_pile.data(), 2 * A.band); })
        && write_file(A.extended_file, "extended consensus", [&](FILE *f) { return write_gapped_consensus(f, R.names, R.extended_starts.data(), R.extended.data()); })
        && write_file(A.extension_report, "extension report", [&](FILE *f) { return write_extension_report(f, R.names, R.ext_pile.data(), A.extend); });
}

static int bait_main(int argc, char **argv)
{
    BaitArgs A;
    if (const int rc = parse_bait_args(argc, argv, A)) return rc;
    mf::cold_mark("fastfilter bait: arguments read");
    BaitResult R;
    mf_kmerset *ks = nullptr; decltype(&mf_kmerset_free) free_set = nullptr;
    if (const int rc = bait_run(A, R, &ks, &free_set)) return rc;
    mf::cold_mark("files filtered");
    if (!write_reports(A, R)) { free_set(ks); return 3; }
    printf("%llu\n", (unsigned long long)R.kept);      // same stdout contract as the contig filter
    // (the outputs are written and closed; what is left is the GPU runtime's teardown -- queues, code objects, a tenth of a second -- which a
    // process that is about to be gone has no use for; a profiler writes its files in a finaliser, so not under one)
    fflush(stdout); fflush(stderr);
    const char *pre = getenv("LD_PRELOAD");
    if (!((pre && strstr(pre, "rocprof")) || getenv("ROCPROFILER_REGISTER_FORCE_LOAD") || getenv("ROCP_TOOL_LIBRARIES"))) _exit(0);
    free_set(ks);
    return 0;
}

// `fastfilter pairs`: the two kept files of a bait step placed as PAIRS (mf_place_pairs; include/mitofilter.h, pairs) -- both files are
// read into memory --, and the reports of the verifying family over both mates plus the pair report.  Prints the rescued mates.
// With --band W the call is mf_align_pairs (include/mitofilter.h, pairs with a band): both files aligned, a rescued mate aligned around
// its seed; --score-report then has the aligned columns, and --indels, --gapped-consensus, --insertions and, with --extend E,
// --extended-consensus and --extension-report are the bait subcommand's files, by its writers and under its dependency rules.  Without
// --band every file and the printed line are what they were.
static int pairs_main(int argc, char **argv)
{
    std::string bait, fq1, fq2, libpath, pair_report, place_report, base_depth_file, consensus_file, score_report;
    std::string indels_file, gapped_file, insertions_file, extended_file, extension_report;
    unsigned long k = 31, min_insert = 0, max_insert = 0, rescue_permille = 100, max_permille = 1000, min_depth = 1, band = 0, extend = 0;
    bool rescue = true, have_band = false;
    static const char *usage = "usage: fastfilter pairs --bait BAIT.fa [-k 31] --fq1 A.fq --fq2 B.fq --min-insert N --max-insert M [--no-rescue] [--rescue-permille 100]\n"
                               "       [--max-mismatch PERMILLE] [--min-depth D] [--pair-report FILE] [--place-report FILE] [--base-depth FILE] [--consensus FILE] [--score-report FILE]\n"
                               "       [--band W [--indels FILE] [--gapped-consensus FILE] [--insertions FILE] [--extend E [--extended-consensus FILE] [--extension-report FILE]]]\n"
                               "       (the files are read into memory: the kept files of a bait step; 1 <= N <= M, at most 4096 inserts wide)\n";
    for (int a = 2; a < argc; a++) {
        const std::string o = argv[a];
        auto need = [&](const char *name) -> std::string {
            if (a + 1 >= argc) { fprintf(stderr, "error: %s requires a value\n", name); exit(1); }
            return argv[++a];
        };
        auto number = [&](const char *name, unsigned long lo, unsigned long hi, unsigned long &out) {
            const std::string v = need(name); char *end = nullptr; const unsigned long x = strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] < '0' || v[0] > '9' || x < lo || x > hi) { fprintf(stderr, "error: %s wants a number from %lu to %lu\n", name, lo, hi); exit(1); }
            out = x;
        };
        if (o == "--bait") bait = need("--bait");
        else if (o == "--fq1") fq1 = need("--fq1");
        else if (o == "--fq2") fq2 = need("--fq2");
        else if (o == "--lib") libpath = need("--lib");
        else if (o == "-k" || o == "--kmer") number("-k", 1, 64, k);
        else if (o == "--min-insert") number("--min-insert", 1, 0x7FFFFFFFul, min_insert);
        else if (o == "--max-insert") number("--max-insert", 1, 0x7FFFFFFFul, max_insert);
        else if (o == "--no-rescue") rescue = false;
        else if (o == "--rescue-permille") number("--rescue-permille", 0, 1000, rescue_permille);
        else if (o == "--max-mismatch") number("--max-mismatch", 0, 1000, max_permille);
        else if (o == "--min-depth") number("--min-depth", 1, 0xFFFFFFFFul, min_depth);
        else if (o == "--pair-report") pair_report = need("--pair-report");
        else if (o == "--place-report") place_report = need("--place-report");
        else if (o == "--base-depth") base_depth_file = need("--base-depth");
        else if (o == "--consensus") consensus_file = need("--consensus");
        else if (o == "--score-report") score_report = need("--score-report");
        else if (o == "--band") { number("--band", 0, 31, band); have_band = true; }
        else if (o == "--indels") indels_file = need("--indels");
        else if (o == "--gapped-consensus") gapped_file = need("--gapped-consensus");
        else if (o == "--insertions") insertions_file = need("--insertions");
        else if (o == "--extend") number("--extend", 1, MF_EXTEND_MAX, extend);
        else if (o == "--extended-consensus") extended_file = need("--extended-consensus");
        else if (o == "--extension-report") extension_report = need("--extension-report");
        else { fprintf(stderr, "error: unknown option '%s' for fastfilter pairs\n", o.c_str()); return 1; }
    }
    if (bait.empty() || fq1.empty() || fq2.empty() || !min_insert || !max_insert) { fputs(usage, stderr); return 1; }
    if (max_insert < min_insert || max_insert - min_insert + 1 > MF_RESCUE_MAX) {
        fprintf(stderr, "error: --min-insert .. --max-insert is a window of 1 to %d inserts\n", MF_RESCUE_MAX);
        return 1;
    }
    // the bait subcommand's dependency rules
    const bool gap = !gapped_file.empty() || !insertions_file.empty();
    if (gap && !have_band) { fprintf(stderr, "error: --gapped-consensus and --insertions need --band\n"); return 1; }
    if ((!extended_file.empty() || !extension_report.empty()) && !extend) { fprintf(stderr, "error: --extended-consensus and --extension-report need --extend\n"); return 1; }
    if (extend && !have_band) { fprintf(stderr, "error: --extend needs --band (--band 0 is fine)\n"); return 1; }
    if (!indels_file.empty() && !have_band) { fprintf(stderr, "error: --indels needs --band\n"); return 1; }
    if (have_band && band >= k) { fprintf(stderr, "error: --band stays below k (%lu)\n", k); return 1; }
    if (libpath.empty()) { const char *e = getenv("MITOFILTER_LIB"); if (e && *e) libpath = e; }
    if (libpath.empty()) libpath = exe_dir() + "/../libmitofilter_hip.so";
    void *h = dlopen(libpath.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "error: cannot load %s: %s (pair-aware placement has no CPU fallback)\n", libpath.c_str(), dlerror()); return 2; }
#define SYM(name) auto p_##name = (decltype(&name))dlsym(h, #name); if (!p_##name) { fprintf(stderr, "error: %s lacks symbol %s\n", libpath.c_str(), #name); return 2; }
    SYM(mf_abi_version) SYM(mf_last_error) SYM(mf_kmerset_build_from_fasta) SYM(mf_kmerset_free) SYM(mf_reads_from_fastq) SYM(mf_reads_free) SYM(mf_reads_info)
    SYM(mf_kmerset_record_count) SYM(mf_kmerset_record_name) SYM(mf_kmerset_record_starts) SYM(mf_place_pairs)
#undef SYM
    if (p_mf_abi_version() != MF_ABI_VERSION) { fprintf(stderr, "error: ABI version mismatch\n"); return 2; }
    mf_kmerset *ks = nullptr; mf_reads *r1 = nullptr, *r2 = nullptr;
    auto fail = [&]() { fprintf(stderr, "error: %s\n", p_mf_last_error()); if (r2) p_mf_reads_free(r2); if (r1) p_mf_reads_free(r1); if (ks) p_mf_kmerset_free(ks); return 3; };
    if (p_mf_kmerset_build_from_fasta(bait.c_str(), (int)k, 0, &ks) != MF_OK) return fail();
    if (p_mf_reads_from_fastq(fq1.c_str(), 0, &r1) != MF_OK || p_mf_reads_from_fastq(fq2.c_str(), 0, &r2) != MF_OK) return fail();
    std::vector<std::string> names; std::vector<uint64_t> starts;
    if (fetch_names(ks, p_mf_kmerset_record_count, p_mf_kmerset_record_name, names) != MF_OK || fetch_starts(ks, p_mf_kmerset_record_starts, names.size(), starts) != MF_OK) return fail();
    const size_t positions = (size_t)std::max<uint64_t>(starts.back(), 1), n_rec = std::max<size_t>(names.size(), 1);
    std::vector<uint32_t> depth(positions, 0); std::vector<uint8_t> consensus(positions, 0);
    std::vector<mf_place_record_t> place_recs(n_rec); std::vector<mf_score_record_t> score_recs(n_rec); std::vector<mf_pair_record_t> pair_recs(n_rec);
    uint64_t none = 0, unplaced[2] = {0, 0};
    std::vector<mf_align_record_t> align_recs; std::vector<mf_indel_t> indels; std::vector<mf_pileup_t> ins_pile, ext_pile;
    std::vector<uint8_t> gapped, extended; std::vector<uint64_t> gapped_starts, extended_starts;
    if (have_band) {
#define SYM(name) auto p_##name = (decltype(&name))dlsym(h, #name); if (!p_##name) { fprintf(stderr, "error: %s lacks symbol %s\n", libpath.c_str(), #name); return 2; }
        SYM(mf_align_pairs)
#undef SYM
        const size_t span = 2 * (size_t)band, E = extend;
        align_recs.assign(n_rec, mf_align_record_t{}); indels.assign(positions, mf_indel_t{});
        if (gap) { ins_pile.assign(std::max<size_t>(positions * span, 1), mf_pileup_t{}); gapped.assign(positions * (1 + span), 0); gapped_starts.assign(n_rec + 1, 0); }
        if (E) { ext_pile.assign(n_rec * 2 * E, mf_pileup_t{}); extended.assign(positions * (1 + span) + 2 * n_rec * E, 0); extended_starts.assign(n_rec + 1, 0); }
        if (p_mf_align_pairs(ks, r1, r2, 1, MF_MODE_SCREENED, (uint32_t)min_depth, (uint32_t)max_permille, (uint32_t)band, (uint32_t)extend, (uint32_t)min_insert,
                             (uint32_t)max_insert, rescue ? 1 : 0, (uint32_t)rescue_permille, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, depth.data(),
                             place_recs.data(), nullptr, consensus_file.empty() ? nullptr : consensus.data(), nullptr, indels.data(), align_recs.data(),
                             gap && span ? ins_pile.data() : nullptr, gap ? gapped.data() : nullptr, gap ? gapped_starts.data() : nullptr, nullptr,
                             E ? ext_pile.data() : nullptr, E ? extended.data() : nullptr, E ? extended_starts.data() : nullptr, nullptr, pair_recs.data(), &none, unplaced,
                             nullptr) != MF_OK) return fail();
    } else
    if (p_mf_place_pairs(ks, r1, r2, 1, MF_MODE_SCREENED, (uint32_t)min_depth, (uint32_t)max_permille, (uint32_t)min_insert, (uint32_t)max_insert, rescue ? 1 : 0,
                         (uint32_t)rescue_permille, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, depth.data(), place_recs.data(), nullptr,
                         consensus_file.empty() ? nullptr : consensus.data(), nullptr, score_recs.data(), pair_recs.data(), &none, unplaced, nullptr) != MF_OK) return fail();
    using namespace mf_text;
    const bool ok = write_file(pair_report, "pair report", [&](FILE *f) { return write_pair_report(f, names, starts, pair_recs.data(), none); })
        && write_file(place_report, "placement report", [&](FILE *f) { return write_place_report(f, names, starts, place_recs.data(), depth.data(), unplaced[0]); })
        && write_file(base_depth_file, "base depth", [&](FILE *f) { return write_base_depth(f, names, starts, depth.data()); })
        && write_file(consensus_file, "consensus", [&](FILE *f) { return write_consensus(f, names, starts, consensus.data()); })
        && write_file(score_report, "score report", [&](FILE *f) { return have_band ? write_align_report(f, names, starts, align_recs.data())
                                                                                    : write_score_report(f, names, starts, score_recs.data()); })
        && write_file(indels_file, "indel table", [&](FILE *f) { return write_indels(f, names, starts, depth.data(), indels.data()); })
        && write_file(gapped_file, "gapped consensus", [&](FILE *f) { return write_gapped_consensus(f, names, gapped_starts.data(), gapped.data()); })
        && write_file(insertions_file, "insertion table", [&](FILE *f) { return write_insertions(f, names, starts, depth.data(), ins_pile.data(), 2 * (unsigned)band); })
        && write_file(extended_file, "extended consensus", [&](FILE *f) { return write_gapped_consensus(f, names, extended_starts.data(), extended.data()); })
        && write_file(extension_report, "extension report", [&](FILE *f) { return write_extension_report(f, names, ext_pile.data(), (unsigned)extend); });
    unsigned long long rescued = 0;
    for (size_t j = 0; j < names.size(); j++) rescued += pair_recs[j].rescued;
    p_mf_reads_free(r2); p_mf_reads_free(r1); p_mf_kmerset_free(ks);
    if (!ok) return 3;
    printf("%llu\n", rescued);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "bait") == 0) return bait_main(argc, argv);
    if (argc >= 2 && strcmp(argv[1], "pairs") == 0) return pairs_main(argc, argv);
    return contig_filter_main(argc, argv);
}
