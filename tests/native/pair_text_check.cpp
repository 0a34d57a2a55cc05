// The pair report of `fastfilter pairs` (mitoflex_amd/csrc/mf_report_text.h: write_pair_report) written from one case that
// tests/test_pair_text.py gives as plain names and numbers on standard input: the number of records, their names, their R + 1 starts,
// six numbers a record (proper, discordant, cross, rescued, single, insert_sum), the pairs without a settled mate.  Writes argv[1].
#include "../../mitoflex_amd/csrc/mf_report_text.h"

#include <iostream>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    size_t n = 0;
    std::cin >> n;
    mf_text::Names names(n);
    for (auto &s : names) std::cin >> s;
    mf_text::Starts starts(n + 1);
    for (auto &s : starts) std::cin >> s;
    std::vector<mf_pair_record_t> recs(n);
    for (auto &r : recs) std::cin >> r.proper >> r.discordant >> r.cross >> r.rescued >> r.single >> r.insert_sum;
    uint64_t none = 0;
    std::cin >> none;
    if (!std::cin) return 2;
    FILE *f = fopen(argv[1], "w");
    const bool ok = mf_text::write_pair_report(f, names, starts, recs.data(), none);
    if (f) fclose(f);
    return ok && !mf_text::write_pair_report(nullptr, names, starts, recs.data(), none) ? 0 : 1;
}
