// Driver of tests/test_extend_text.py: reads one case (plain names and numbers, whitespace-separated) and writes extended.fa and
// extension.tsv with mf_report_text.h's write_gapped_consensus (which `fastfilter bait --extended-consensus` writes the extended records
// with) and write_extension_report.  Built under ASan + UBSan by the test: the arrays are exactly as large as the case says.
//   extend_text_check CASE OUTDIR
// Case: R; R names; E; R + 1 extended starts; the extended records as one word ("-" when it is empty); then 2 R rows (begin, end of
// every record) of E times A C G T.
#include "../../mitoflex_amd/csrc/mf_report_text.h"

#include <fstream>
#include <iostream>

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: extend_text_check CASE OUTDIR\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t R = 0;
    in >> R;
    mf_text::Names names(R);
    for (auto &n : names) in >> n;
    uint32_t E = 0;
    in >> E;
    mf_text::Starts xstarts(R + 1);
    for (auto &s : xstarts) in >> s;
    std::string word;
    in >> word;
    if (word == "-") word.clear();
    if (word.size() != xstarts[R]) { fprintf(stderr, "extend_text_check: the records do not have the length of their offsets\n"); return 2; }
    std::vector<uint8_t> extended(word.begin(), word.end());
    std::vector<mf_pileup_t> ext(2 * R * E);
    for (auto &c : ext) in >> c.a >> c.c >> c.g >> c.t;
    if (!in) { fprintf(stderr, "extend_text_check: the case is short\n"); return 2; }
    const std::string dir = argv[2];
    FILE *f = fopen((dir + "/extended.fa").c_str(), "w");
    bool ok = mf_text::write_gapped_consensus(f, names, xstarts.data(), extended.data());
    if (f) fclose(f);
    f = fopen((dir + "/extension.tsv").c_str(), "w");
    ok = mf_text::write_extension_report(f, names, ext.data(), E) && ok;
    if (f) fclose(f);
    ok = !mf_text::write_extension_report(nullptr, names, ext.data(), E) && ok;
    printf("the writers returned %s\n", ok ? "true" : "false");
    return 0;
}
