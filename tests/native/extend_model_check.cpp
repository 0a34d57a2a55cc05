// Driver of tests/test_extend_model.py: holds the scalar pieces of the extended records in mitoflex_amd/csrc/mf_call.h -- extend_offset and
// extend_entry, which align_adds stores an overhanging base by, and extend_call_column, which extend_call_kernel calls a column by -- to
// cases that the plain-Python oracle (tests/extend_oracle.py) dumps.  Plain integer code: no device, built plain and under ASan + UBSan;
// every table is exactly as large as its case says.
//   extend_model_check CASES
// A line "P R E j len n  c letter .. (n times)  m  entry letter count .. (m times)": the diagonal steps of one accepted read of record j
// (len positions) that lie outside the record, each its coordinate and letter (0 .. 3, 4 for an N), into a table of R records and E
// columns an end; then the m counters that are not zero, by their index into the flat table of 4 * 2 * R * E.
// A line "C E min_depth  E times a c g t  n letters": one end's table, unclamped; how many columns it emits and their letters ("-": none).
#include "../../mitoflex_amd/csrc/mf_call.h"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: extend_model_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    size_t n_lines = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        n_lines++;
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        if (kind == "P") {
            uint64_t R, E, j, n; int64_t len;
            s >> R >> E >> j >> len >> n;
            std::vector<unsigned long long> table(4 * 2 * R * E, 0);
            for (uint64_t i = 0; i < n; i++) {
                int64_t c; uint32_t letter;
                s >> c >> letter;
                if (c >= 0 && c < len) { fprintf(stderr, "line %zu: a coordinate inside the record\n", n_lines); return 1; }
                uint32_t side;
                const uint64_t off = mf::extend_offset(c, len, side);
                if (off >= E || letter >= 4) continue;          // (what align_adds asks before it stores)
                table.at(4 * mf::extend_entry(j, side, (uint32_t)E, off) + letter)++;
            }
            uint64_t m;
            s >> m;
            std::vector<unsigned long long> want(table.size(), 0);
            for (uint64_t i = 0; i < m; i++) { uint64_t at; unsigned long long v; s >> at >> v; want.at(at) = v; }
            if (!s) { fprintf(stderr, "line %zu is short\n", n_lines); return 2; }
            if (table != want) { fprintf(stderr, "line %zu: the table differs from the oracle's\n", n_lines); return 1; }
        } else if (kind == "C") {
            uint32_t E, min_depth;
            s >> E >> min_depth;
            std::vector<unsigned long long> t(4 * (size_t)E);
            for (auto &v : t) s >> v;
            uint32_t n; std::string letters;
            s >> n >> letters;
            if (!s) { fprintf(stderr, "line %zu is short\n", n_lines); return 2; }
            if (letters == "-") letters.clear();
            std::string got;
            for (uint32_t e = 0; e < E; e++) {          // an end emits its columns up to the first that is not
                uint8_t byte;
                if (!mf::extend_call_column(t[4 * e], t[4 * e + 1], t[4 * e + 2], t[4 * e + 3], min_depth, byte)) break;
                got.push_back((char)byte);
            }
            if (got != letters || got.size() != n) { fprintf(stderr, "line %zu: emitted '%s', the oracle '%s'\n", n_lines, got.c_str(), letters.c_str()); return 1; }
        } else { fprintf(stderr, "line %zu: unknown kind\n", n_lines); return 2; }
    }
    printf("extend model ok: %zu cases\n", n_lines);
    return 0;
}
