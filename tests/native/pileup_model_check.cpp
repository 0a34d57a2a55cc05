// The pile-up's per-position call (mitoflex_amd/csrc/mf_call.h) on the CPU, against cases that the plain-Python oracle
// (tests/pileup_oracle.py) dumps.  Built by tests/test_pileup_model.py, once plain and once with -fsanitize=address,undefined.
//
//   c0 c1 c2 c3  ref  min_depth   consensus called ambiguous variant matches mismatches   the four counters as they are reported
//   ref: the bait's letter, N for an invalid one.  matches / mismatches: what the position adds to its record's sums -- its bases that
//   show the bait's letter and the others, nothing on an invalid letter (as pileup_call_kernel adds them from own and depth).
// Prints "pileup model ok: <cases> cases" and exits 0, or the first difference and exits 1.
#include "../../mitoflex_amd/csrc/mf_call.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace mf;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: pileup_model_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    unsigned long long cases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        unsigned long long c[4], matches, mismatches, clamped[4];
        std::string ref, cons;
        uint32_t min_depth; int called, ambiguous, variant;
        ss >> c[0] >> c[1] >> c[2] >> c[3] >> ref >> min_depth >> cons >> called >> ambiguous >> variant >> matches >> mismatches >> clamped[0] >> clamped[1] >>
            clamped[2] >> clamped[3];
        cases++;
        if (!ss || ref.size() != 1 || cons.size() != 1) { printf("case %llu: cannot be read\n", cases); return 1; }
        const char *f = strchr("ACGT", ref[0]);
        const bool valid = f && *f;
        // (an invalid position's packed letter is whatever the word holds: the call must not look at it)
        for (uint32_t b = valid ? (uint32_t)(f - "ACGT") : 0u; b < 4; b += valid ? 4u : 1u) {
            const PileCall r = pileup_call_position(c[0], c[1], c[2], c[3], b, valid, min_depth);
            const unsigned long long got_matches = valid ? r.own : 0, got_mismatches = valid ? r.depth - r.own : 0;
            if (r.consensus != (uint8_t)cons[0] || (int)r.called != called || (int)r.ambiguous != ambiguous || (int)r.variant != variant ||
                r.depth != c[0] + c[1] + c[2] + c[3] || got_matches != matches || got_mismatches != mismatches) {
                printf("DIFFERS: case %llu (%s): oracle '%s' called %d ambiguous %d variant %d matches %llu mismatches %llu, model '%c' %d %d %d %llu %llu\n", cases,
                       line.c_str(), cons.c_str(), called, ambiguous, variant, matches, mismatches, (char)r.consensus, (int)r.called, (int)r.ambiguous,
                       (int)r.variant, got_matches, got_mismatches);
                return 1;
            }
        }
        for (int l = 0; l < 4; l++)
            if (clamp_count(c[l]) != clamped[l]) { printf("DIFFERS: case %llu: counter %d of %llu is reported as %u, oracle %llu\n", cases, l, c[l], clamp_count(c[l]), clamped[l]); return 1; }
    }
    printf("pileup model ok: %llu cases\n", cases);
    return 0;
}
