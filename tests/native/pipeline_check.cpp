// The file pipeline (readers, pools, pack, ordered writers) with a stand-in filter on the CPU, so that it can run
// under sanitizers and without a GPU: a read passes iff its first base is A/a.
//   pipeline_check FQ1 FQ2|- OUT1 OUT2|- BATCH_READS PACK_THREADS [both|either [N_DEVICES [report]]]   -> prints "kept total"
// With N_DEVICES > 1 the stand-in filter sleeps a pseudo-random time that depends on the device and the batch, so that
// batches come back out of order and the dealing / reordering logic of run_fastq_pipeline is exercised.
// With `report` the pipeline is given a stand-in report, whose hook it calls behind every pass: a passing read at
// index i of its batch goes to record i % 4 of three (3: no record wins), and the tally follows on a second line:
// "tally c0 c1 c2 ambiguous unassigned".
#include "mf_pipeline.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <thread>
// the batch the calling worker thread has just filtered: what the stand-in hook is asked about (the library's holds a read set instead)
struct Held { const std::vector<uint32_t> *bits; uint64_t n; };
static thread_local Held t_held{nullptr, 0};
int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const char *fq2 = strcmp(argv[2], "-") ? argv[2] : nullptr, *out2 = strcmp(argv[4], "-") ? argv[4] : nullptr;
    const int n_devices = argc > 8 ? atoi(argv[8]) : 1;
    std::atomic<unsigned> calls{0};
    struct FakeReport : mf::PassReport {
        FakeReport() : PassReport(3) {}
        int after_pass(mf_reads *, std::vector<uint64_t> &pairs, std::string &) override
        {
            for (uint64_t i = 0; i < t_held.n; i++)
                if (((*t_held.bits)[i >> 5] >> (i & 31)) & 1) pairs.push_back(i << 32 | (i % 4 < 3 ? i % 4 : 0xFFFFFFFEu));
            return 0;
        }
    } fake;
    mf::PassReport *report = argc > 9 && !strcmp(argv[9], "report") ? &fake : nullptr;
    fake.held.assign((size_t)n_devices, nullptr);          // (the stand-in has no read sets: its hook looks at t_held)
    mf::BatchFilterFn fn = [n_devices, &calls](int device, const mf::PackedHost &P, uint64_t n, std::vector<uint32_t> &bits, std::string &) -> int {
        if (n_devices > 1) {
            const unsigned c = calls.fetch_add(1);
            std::this_thread::sleep_for(std::chrono::microseconds(((c * 2654435761u) >> 20) % 3000 + (device % 3) * 500));
        }
        bits.assign((n + 31) / 32 + 1, 0);
        size_t ni = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t g = P.offsets[i];
            while (ni < P.npos.size() && P.npos[ni] < g) ni++;
            const bool invalid = ni < P.npos.size() && P.npos[ni] == g;
            if (P.offsets[i + 1] > g && !invalid && ((P.words[g >> 4] >> (2 * (g & 15))) & 3u) == 0) bits[i >> 5] |= 1u << (i & 31);
        }
        t_held = Held{&bits, n};
        return 0;
    };
    mf::PipelineStats st; std::string err;
    const int rc = mf::run_fastq_pipeline(argv[1], fq2, argv[3], out2, argc > 7 && !strcmp(argv[7], "both"), n_devices, atoi(argv[6]),
                                          strtoull(argv[5], nullptr, 10), fn, st, err, report);
    if (rc) { printf("error %d: %s\n", rc, err.c_str()); return 0; }
    printf("%llu %llu\n", (unsigned long long)st.kept, (unsigned long long)st.total);
    if (report) { printf("tally"); for (const uint64_t c : report->counts) printf(" %llu", (unsigned long long)c); printf("\n"); }
    return 0;
}
