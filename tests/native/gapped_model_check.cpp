// The gapped consensus' scalar pieces (mitoflex_amd/csrc/mf_align.h, mf_call.h) on the CPU, against cases that the plain-Python oracle
// (tests/gapped_oracle.py) dumps.  Built by tests/test_gapped_model.py, once plain and once with -fsanitize=address,undefined: the
// insertion pile is an exactly-sized heap array, so a store behind a position's own entries at the end of the bait stops the program.
//
//   R  the run-offset walk (align_run_offset) over the words the traceback leaves per read base, and the store align_adds makes from
//      it: for an inserted base whose position c - 1 lies in [0, len), one add at [(s0 + c - 1) * span + t][letter] when t < span and the
//      letter is one.  The whole pile must equal the oracle's.
//      R span s0 len total L x  ent[0] .. ent[L-1]  n  (position offset letter count) x n
//   C  the call at one position (gapped_call_position): the emitted bytes and whether the position is deleted.
//      C span min_depth D del cons  4 * span counters  deleted bytes   ("-" for no byte)
// Prints "gapped model ok: <cases> cases" and exits 0, or the first difference and exits 1.
#include "../../mitoflex_amd/csrc/mf_align.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace mf;

struct Pile {
    unsigned long long *w; size_t n;
    explicit Pile(size_t n_) : w((unsigned long long *)calloc(n_ ? n_ : 1, 8)), n(n_) {}
    ~Pile() { free(w); }
    Pile(const Pile &) = delete;
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: gapped_model_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    unsigned long long cases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        cases++;
        if (kind == "R") {
            uint32_t span; uint64_t s0, total, L; long long len; std::string x; size_t n;
            ss >> span >> s0 >> len >> total >> L >> x;
            std::vector<unsigned long long> ent(L);
            for (auto &e : ent) ss >> e;
            ss >> n;
            Pile want((size_t)total * span * 4), got((size_t)total * span * 4);
            for (size_t q = 0; q < n; q++) {
                uint64_t p; uint32_t t, letter; unsigned long long c;
                ss >> p >> t >> letter >> c;
                if (ss && p < total && t < span && letter < 4) want.w[4 * (p * span + t) + letter] += c;
            }
            if (!ss || x.size() != L) { printf("case %llu: cannot be read\n", cases); return 1; }
            for (uint64_t b = 0; b < L; b++) {                      // what align_adds does with an inserted base
                const unsigned long long e = ent[b];
                const long long p = (long long)(int32_t)(uint32_t)e - 1;
                if (p < 0 || p >= len || !((e >> 32) & 1u)) continue;
                const uint32_t t = align_run_offset(ent.data(), b, span);
                const char *f = strchr("ACGT", x[b]);
                if (t < span && f && *f) got.w[4 * ((s0 + (uint64_t)p) * span + t) + (uint32_t)(f - "ACGT")] += 1;
            }
            if (memcmp(want.w, got.w, want.n * 8) != 0) {
                printf("DIFFERS: case %llu (walk, span %u L %llu)\n", cases, span, (unsigned long long)L);
                for (size_t i = 0; i < want.n; i++) if (want.w[i] != got.w[i]) printf("  [%zu offset %zu letter %zu] oracle %llu model %llu\n", i / (4 * span), i / 4 % span, i % 4, want.w[i], got.w[i]);
                return 1;
            }
        } else if (kind == "C") {
            uint32_t span, min_depth; unsigned long long D, del; std::string cons, bytes; int deleted;
            ss >> span >> min_depth >> D >> del >> cons;
            Pile ins((size_t)span * 4);
            for (size_t i = 0; i < ins.n; i++) ss >> ins.w[i];
            ss >> deleted >> bytes;
            if (!ss || cons.size() != 1) { printf("case %llu: cannot be read\n", cases); return 1; }
            if (bytes == "-") bytes.clear();
            std::vector<uint8_t> out(1 + span);                    // exactly the room the caller's scratch has
            bool was_deleted = false;
            const uint32_t m = gapped_call_position(D, del, span ? ins.w : nullptr, span, min_depth, (uint8_t)cons[0], out.data(), was_deleted);
            if (m > 1 + span || std::string(out.begin(), out.begin() + m) != bytes || (int)was_deleted != deleted) {
                printf("DIFFERS: case %llu (call): oracle '%s' deleted %d, model '%s' deleted %d\n", cases, bytes.c_str(), deleted,
                       std::string(out.begin(), out.begin() + (m <= 1 + span ? m : 0)).c_str(), (int)was_deleted);
                return 1;
            }
        } else { printf("case %llu: unknown kind\n", cases); return 1; }
    }
    printf("gapped model ok: %llu cases\n", cases);
    return 0;
}
