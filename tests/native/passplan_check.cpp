// Driver of tests/test_passplan.py: the pass plan, the tally layout and the feedback of mitoflex_amd/csrc/mf_passplan.h are pure host code, so
// they are run here without a device (ASan + UBSan).  Reads rows of integers from the file named on the command line, writes one answer a row:
//   plan <6 knobs> <17 inputs>          the plan of one pass
//   seq <n> <6 knobs> <17 inputs>       n plans, each pass's flip and cur fed into the next
//   layout                              words, bytes and the word offsets of the three regions
//   sum <regions>                       the two totals of a block whose word i holds 3 * i + 1
//   adapt <prefer_split> <finish_two> <split_serial> <sample_pass> <cand> <n_reads>
// knobs: pass finish_streams screen_streams split_pipe exact_co s8_finish; inputs: prot s stride kw k s8_finish thr mode count_all overlap more
// prefer_split finish_two split_serial flip cur nsets
#include "../../mitoflex_amd/csrc/mf_passplan.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace mf;

static bool read_case(FILE *f, PassKnobs &kn, PassInputs &in)
{
    int v[23];
    for (int &x : v) if (fscanf(f, "%d", &x) != 1) return false;
    kn = PassKnobs{v[0], v[1], v[2], v[3], v[4], v[5]};
    in = PassInputs{v[6], v[7], v[8], v[9], v[10], v[11], (unsigned)v[12], v[13], v[14] != 0, v[15] != 0, v[16] != 0,
                    PassFeedback{v[17] != 0, v[18] != 0, v[19] != 0}, v[20], v[21], v[22]};
    return true;
}

static void print_plan(const PassPlan &p)
{
    static const char *const kinds[] = {"PROTEIN", "FINISH", "SPLIT_PIPELINED", "ONE_STREAM"}, *const streams[] = {"MAIN", "FINISH_A", "SCREEN_ALT", "FINISH_B"};
    printf("%s %d %d %d %s %s %d %d %d %d %d %d %d %d %d %d\n", kinds[(int)p.kind], (int)p.two_streams, p.q, p.q_out, streams[(int)p.screen_on], streams[(int)p.later_on],
           (int)p.screen, (int)p.wait_prev_finish, (int)p.screen_clears_bits, (int)p.needs_cand, (int)p.exact_behind_finish, (int)p.exact_coresident, p.flip, p.cur,
           (int)p.sample_pass, p.tally_regions);
}

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: passplan_check ROWS\n"); return 2; }
    char cmd[16];
    PassKnobs kn; PassInputs in;
    while (fscanf(f, "%15s", cmd) == 1) {
        if (!strcmp(cmd, "plan")) {
            if (!read_case(f, kn, in)) return 3;
            print_plan(plan_pass(kn, in));
        } else if (!strcmp(cmd, "seq")) {
            int n = 0;
            if (fscanf(f, "%d", &n) != 1 || !read_case(f, kn, in)) return 3;
            for (int i = 0; i < n; i++) { const PassPlan p = plan_pass(kn, in); print_plan(p); in.flip = p.flip; in.cur = p.cur; }
        } else if (!strcmp(cmd, "layout")) {
            printf("%zu %zu %zu %zu %zu\n", TallyLayout::words(), TallyLayout::bytes(), TallyLayout::region(0), TallyLayout::region(1), TallyLayout::region(2));
        } else if (!strcmp(cmd, "sum")) {
            int regions = 0;
            if (fscanf(f, "%d", &regions) != 1 || regions < 0 || regions > TallyLayout::REGIONS) return 3;
            std::vector<unsigned long long> block(TallyLayout::words());          // (exactly a block: a sum that reads past it is an ASan report)
            for (size_t i = 0; i < block.size(); i++) block[i] = 3 * i + 1;
            const TallyLayout::Totals t = TallyLayout::sum(block.data(), regions);
            printf("%llu %llu\n", t.pass, t.cand);
        } else if (!strcmp(cmd, "adapt")) {
            int a, b, c, sample; unsigned long long cand, n_reads;
            if (fscanf(f, "%d %d %d %d %llu %llu", &a, &b, &c, &sample, &cand, &n_reads) != 6) return 3;
            const PassFeedback fb = adapt_after_call(PassFeedback{a != 0, b != 0, c != 0}, sample != 0, cand, n_reads);
            printf("%d %d %d\n", (int)fb.prefer_split, (int)fb.finish_two, (int)fb.split_serial);
        } else return 3;
    }
    fclose(f);
    return 0;
}
