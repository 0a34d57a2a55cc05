// The keep rule on the host pipeline with a stand-in filter and a stand-in report on the CPU, so that it can run under sanitizers and
// without a GPU (in the manner of pipeline_check.cpp): a read passes iff its first base is A/a.
//   keep_check FQ1 FQ2|- OUT1 OUT2|- BATCH_READS PACK_THREADS both|either N_DEVICES KEEP   -> prints "kept total"
// The stand-in report overrides amend_bits, the one door through which a report changes what the pair rule sees: a passing read whose
// second base is C/c counts as "placed and rejected by the cut", one whose second base is G/g as "not placed", every other one as
// placed and accepted; the bit is cleared where mf_score.h's keep_clears says so for the keep mode KEEP (0, 1, 2).  With N_DEVICES > 1
// the stand-in filter sleeps a pseudo-random time, so that the workers' batches come back out of order.
#include "mf_pipeline.h"
#include "mf_score.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
// the batch the calling worker thread has just filtered: what the stand-in hooks are asked about (the library's hold a read set instead)
static thread_local const mf::PackedHost *t_held = nullptr;
static thread_local uint64_t t_held_n = 0;
// base j of read i of the batch: 0 .. 3 for A C G T, -1 where the read has no such base or it is not a valid letter
static int base_at(const mf::PackedHost &P, uint64_t i, uint64_t j)
{
    const uint64_t g = P.offsets[i] + j;
    if (g >= P.offsets[i + 1]) return -1;
    if (std::binary_search(P.npos.begin(), P.npos.end(), g)) return -1;
    return (int)((P.words[g >> 4] >> (2 * (g & 15))) & 3u);
}
int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const char *fq2 = strcmp(argv[2], "-") ? argv[2] : nullptr, *out2 = strcmp(argv[4], "-") ? argv[4] : nullptr;
    const int n_devices = atoi(argv[8]), keep = atoi(argv[9]);
    std::atomic<unsigned> calls{0};
    struct KeepReport : mf::PassReport {
        const int keep;
        std::atomic<uint64_t> amended{0};
        explicit KeepReport(int keep_) : PassReport(0, false), keep(keep_) {}
        int after_pass(mf_reads *, std::vector<uint64_t> &, std::string &) override { return 0; }
        int amend_bits(mf_reads *, uint32_t *bits, uint64_t n, std::string &err) override
        {
            if (!t_held || n != t_held_n) { err = "amend_bits was not called behind this thread's pass"; return 1; }
            for (uint64_t i = 0; i < n; i++) {
                if (!((bits[i >> 5] >> (i & 31)) & 1u)) continue;
                const int b = base_at(*t_held, i, 1);
                if (mf::keep_clears(/*placed*/ b != 2, /*accepted*/ b != 1, keep)) bits[i >> 5] &= ~(1u << (i & 31));
            }
            t_held = nullptr;
            amended++;
            return 0;
        }
    } report(keep);
    report.held.assign((size_t)n_devices, nullptr);          // (the stand-in has no read sets: its hooks look at t_held)
    mf::BatchFilterFn fn = [n_devices, &calls](int device, const mf::PackedHost &P, uint64_t n, std::vector<uint32_t> &bits, std::string &) -> int {
        if (n_devices > 1) {
            const unsigned c = calls.fetch_add(1);
            std::this_thread::sleep_for(std::chrono::microseconds(((c * 2654435761u) >> 20) % 3000 + (device % 3) * 500));
        }
        bits.assign((n + 31) / 32 + 1, 0);
        for (uint64_t i = 0; i < n; i++) if (base_at(P, i, 0) == 0) bits[i >> 5] |= 1u << (i & 31);
        t_held = &P; t_held_n = n;
        return 0;
    };
    mf::PipelineStats st; std::string err;
    const int rc = mf::run_fastq_pipeline(argv[1], fq2, argv[3], out2, !strcmp(argv[7], "both"), n_devices, atoi(argv[6]), strtoull(argv[5], nullptr, 10), fn, st,
                                          err, &report);
    if (rc) { printf("error %d: %s\n", rc, err.c_str()); return 0; }
    printf("%llu %llu\n", (unsigned long long)st.kept, (unsigned long long)st.total);
    printf("amended %llu of %llu\n", (unsigned long long)report.amended.load(), (unsigned long long)(st.batches * (fq2 ? 2 : 1)));
    return 0;
}
