// Driver of tests/test_align_abi.py: reads one case (plain names and numbers, whitespace-separated) and writes align.tsv and indels.tsv
// with mf_report_text.h's write_align_report and write_indels, the functions `fastfilter bait --band W --score-report / --indels` writes
// the files with.  Built under ASan + UBSan by the test: the arrays are exactly as large as the case says.
//   align_text_check CASE OUTDIR
// Case: R; R names; R + 1 starts; R rows of accepted rejected compared mismatches insertions deletions gapped and MF_SCORE_BINS bins;
// then starts[R] rows of depth del ins ins_bases.
#include "../../mitoflex_amd/csrc/mf_report_text.h"

#include <fstream>
#include <iostream>

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: align_text_check CASE OUTDIR\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t R = 0;
    in >> R;
    mf_text::Names names(R);
    for (auto &n : names) in >> n;
    mf_text::Starts starts(R + 1);
    for (auto &s : starts) in >> s;
    std::vector<mf_align_record_t> recs(R);
    for (auto &d : recs) {
        in >> d.accepted >> d.rejected >> d.compared >> d.mismatches >> d.insertions >> d.deletions >> d.gapped;
        for (int b = 0; b < MF_SCORE_BINS; b++) in >> d.hist[b];
    }
    std::vector<uint32_t> depth(starts[R]);
    std::vector<mf_indel_t> indels(starts[R]);
    for (size_t p = 0; p < depth.size(); p++) in >> depth[p] >> indels[p].del >> indels[p].ins >> indels[p].ins_bases;
    if (!in) { fprintf(stderr, "align_text_check: the case is short\n"); return 2; }
    const std::string dir = argv[2];
    FILE *f = fopen((dir + "/align.tsv").c_str(), "w");
    bool ok = mf_text::write_align_report(f, names, starts, recs.data());
    if (f) fclose(f);
    f = fopen((dir + "/indels.tsv").c_str(), "w");
    ok = mf_text::write_indels(f, names, starts, depth.data(), indels.data()) && ok;
    if (f) fclose(f);
    ok = !mf_text::write_align_report(nullptr, names, starts, recs.data()) && !mf_text::write_indels(nullptr, names, starts, depth.data(), indels.data()) && ok;
    printf("the writers returned %s\n", ok ? "true" : "false");
    return 0;
}
