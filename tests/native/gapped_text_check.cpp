// Driver of tests/test_gapped_abi.py: reads one case (plain names and numbers, whitespace-separated) and writes gapped.fa and
// insertions.tsv with mf_report_text.h's write_gapped_consensus and write_insertions, the functions `fastfilter bait --band W
// --gapped-consensus / --insertions` writes the files with.  Built under ASan + UBSan by the test: the arrays are exactly as large as
// the case says.
//   gapped_text_check CASE OUTDIR
// Case: R; R names; R + 1 starts; span; R + 1 gapped starts; the gapped consensus as one word ("-" when it is empty); then starts[R] rows
// of depth and span times A C G T.
#include "../../mitoflex_amd/csrc/mf_report_text.h"

#include <fstream>
#include <iostream>

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: gapped_text_check CASE OUTDIR\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t R = 0;
    in >> R;
    mf_text::Names names(R);
    for (auto &n : names) in >> n;
    mf_text::Starts starts(R + 1), gstarts(R + 1);
    for (auto &s : starts) in >> s;
    uint32_t span = 0;
    in >> span;
    for (auto &s : gstarts) in >> s;
    std::string word;
    in >> word;
    if (word == "-") word.clear();
    if (word.size() != gstarts[R]) { fprintf(stderr, "gapped_text_check: the consensus does not have the length of its offsets\n"); return 2; }
    std::vector<uint8_t> gapped(word.begin(), word.end());
    std::vector<uint32_t> depth(starts[R]);
    std::vector<mf_pileup_t> ins(starts[R] * span);
    for (size_t p = 0; p < depth.size(); p++) {
        in >> depth[p];
        for (uint32_t q = 0; q < span; q++) { mf_pileup_t &c = ins[p * span + q]; in >> c.a >> c.c >> c.g >> c.t; }
    }
    if (!in) { fprintf(stderr, "gapped_text_check: the case is short\n"); return 2; }
    const std::string dir = argv[2];
    FILE *f = fopen((dir + "/gapped.fa").c_str(), "w");
    bool ok = mf_text::write_gapped_consensus(f, names, gstarts.data(), gapped.data());
    if (f) fclose(f);
    f = fopen((dir + "/insertions.tsv").c_str(), "w");
    ok = mf_text::write_insertions(f, names, starts, depth.data(), ins.data(), span) && ok;
    if (f) fclose(f);
    ok = !mf_text::write_gapped_consensus(nullptr, names, gstarts.data(), gapped.data()) && !mf_text::write_insertions(nullptr, names, starts, depth.data(), ins.data(), span) && ok;
    printf("the writers returned %s\n", ok ? "true" : "false");
    return 0;
}
