// Driver of tests/test_score_text.py: reads one case (plain names and numbers, whitespace-separated) and writes score.tsv with
// mf_report_text.h's write_score_report, the function `fastfilter bait --score-report` writes the file with.  Built under ASan + UBSan
// by the test: the arrays are exactly as large as the case says.
//   score_text_check CASE OUTDIR            writes OUTDIR/score.tsv
//   score_text_check CASE --unwritable P    the writer on a file that cannot be opened or written: it must return false
// Case: R; R names; R + 1 starts; R rows of accepted rejected compared mismatches and MF_SCORE_BINS bins.
#include "../../mitoflex_amd/csrc/mf_report_text.h"

#include <cstring>
#include <fstream>
#include <iostream>

int main(int argc, char **argv)
{
    if (argc != 3 && !(argc == 4 && !strcmp(argv[2], "--unwritable"))) { fprintf(stderr, "usage: score_text_check CASE OUTDIR | CASE --unwritable PATH\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t R = 0;
    in >> R;
    mf_text::Names names(R);
    for (auto &n : names) in >> n;
    mf_text::Starts starts(R + 1);
    for (auto &s : starts) in >> s;
    std::vector<mf_score_record_t> recs(R);
    for (auto &d : recs) {
        in >> d.accepted >> d.rejected >> d.compared >> d.mismatches;
        for (int b = 0; b < MF_SCORE_BINS; b++) in >> d.hist[b];
    }
    if (!in) { fprintf(stderr, "score_text_check: the case is short\n"); return 2; }
    const std::string path = argc == 4 ? std::string(argv[3]) : std::string(argv[2]) + "/score.tsv";
    FILE *f = fopen(path.c_str(), "w");
    const bool ok = mf_text::write_score_report(f, names, starts, recs.data());
    if (f) fclose(f);
    printf("write_score_report returned %s\n", ok ? "true" : "false");
    return 0;
}
