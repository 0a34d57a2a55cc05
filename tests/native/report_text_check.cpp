// Driver of tests/test_report_text.py for the report writers of `fastfilter bait` (mitoflex_amd/csrc/mf_report_text.h), which need no
// device:  report_text_check CASE OUTDIR  reads one case -- white-space separated names and numbers, in the order read below, written
// by the test -- and writes all eight formats into OUTDIR;  report_text_check CASE --unwritable PATH  hands every writer what fopen
// makes of PATH and reports whether each returned false.
#include "../../mitoflex_amd/csrc/mf_report_text.h"

using namespace mf_text;

static FILE *g_in;
static bool g_bad = false;
static ull num() { ull v = 0; if (fscanf(g_in, "%llu", &v) != 1) g_bad = true; return v; }
static std::string word() { char b[256]; if (fscanf(g_in, "%255s", b) != 1) { g_bad = true; return ""; } return b; }
static Names words(size_t n) { Names v; for (size_t i = 0; i < n; i++) v.push_back(word()); return v; }
template <class T> static std::vector<T> nums(size_t n) { std::vector<T> v; for (size_t i = 0; i < n; i++) v.push_back((T)num()); return v; }
static std::vector<uint8_t> letters_of(size_t n) { const std::string s = n ? word() : ""; if (s.size() != n) g_bad = true; return std::vector<uint8_t>(s.begin(), s.end()); }

int main(int argc, char **argv)
{
    if (argc < 3 || !(g_in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: report_text_check CASE (OUTDIR | --unwritable PATH)\n"); return 2; }
    const size_t n_rec = (size_t)num();
    const Names names = words(n_rec);
    const Starts starts = nums<uint64_t>(n_rec + 1);
    if (g_bad || starts.empty()) { fprintf(stderr, "the case does not start with its records\n"); return 2; }
    const size_t positions = (size_t)starts.back();
    const std::vector<uint64_t> record_reads = nums<uint64_t>(n_rec + 2);
    const size_t n_grp = (size_t)num();
    const Names groups = words(n_grp);
    const std::vector<uint64_t> group_reads = nums<uint64_t>(n_grp + 2);
    std::vector<mf_depth_record_t> depth_recs;
    for (size_t i = 0; i < n_rec; i++) { const ull w = num(), c = num(), s = num(), m = num(); depth_recs.push_back(mf_depth_record_t{w, c, s, m}); }
    const std::vector<uint32_t> profile = nums<uint32_t>(positions);
    std::vector<mf_place_record_t> place_recs;
    for (size_t i = 0; i < n_rec; i++) { const ull f = num(), r = num(), b = num(), e = num(), c = num(), s = num(); place_recs.push_back(mf_place_record_t{f, r, b, e, c, s}); }
    const std::vector<uint32_t> base_depth = nums<uint32_t>(positions);
    const uint64_t not_placed = num();
    const std::vector<uint8_t> letters = letters_of(positions);
    std::vector<mf_pileup_t> pile;
    for (size_t p = 0; p < positions; p++) { const uint32_t a = (uint32_t)num(), c = (uint32_t)num(), g = (uint32_t)num(), t = (uint32_t)num(); pile.push_back(mf_pileup_t{a, c, g, t}); }
    const std::vector<uint8_t> consensus = letters_of(positions);
    if (g_bad || fscanf(g_in, "%*s") != EOF) { fprintf(stderr, "the case is short, long or malformed\n"); return 2; }
    fclose(g_in);

    const bool unwritable = std::string(argv[2]) == "--unwritable";
    if (unwritable && argc < 4) return 2;
    int failed = 0;
    auto run = [&](const char *file, auto write) {
        const std::string path = unwritable ? std::string(argv[3]) : std::string(argv[2]) + "/" + file;
        FILE *f = fopen(path.c_str(), "w");
        bool ok = write(f);
        if (f) ok = fclose(f) == 0 && ok;
        if (!ok) failed++;
        printf("%s: the writer returned %s\n", file, ok ? "true" : "false");
    };
    run("reads.tsv", [&](FILE *f) { return write_reads(f, false, names, record_reads.data()); });
    run("groups.tsv", [&](FILE *f) { return write_reads(f, true, groups, group_reads.data()); });
    run("depth_report.tsv", [&](FILE *f) { return write_depth_report(f, names, starts, depth_recs.data()); });
    run("depth_profile.tsv", [&](FILE *f) { return write_depth_profile(f, names, starts, profile.data()); });
    run("place_report.tsv", [&](FILE *f) { return write_place_report(f, names, starts, place_recs.data(), base_depth.data(), not_placed); });
    run("base_depth.tsv", [&](FILE *f) { return write_base_depth(f, names, starts, base_depth.data()); });
    run("pileup.tsv", [&](FILE *f) { return write_pileup(f, names, starts, letters.data(), pile.data()); });
    run("consensus.fa", [&](FILE *f) { return write_consensus(f, names, starts, consensus.data()); });
    run("variants.tsv", [&](FILE *f) { return write_variants(f, names, starts, letters.data(), pile.data(), consensus.data()); });
    return unwritable ? (failed == 9 ? 0 : 1) : (failed ? 1 : 0);
}
