// Chunked FASTQ -> pack -> GPU -> survivors pipeline behind mf_filter_fastq_files.
// Stages run on their own threads and overlap: inflate/read + parse (one reader per mate),
// 2-bit pack, H2D + kernels (one worker per device, batches of whole pairs dealt round robin,
// no collective), ordered write-out (one writer per output file).
#pragma once
#include "mf_host.h"
#include <functional>
#include <mutex>
#include <string>
#include <vector>

struct mf_reads;

namespace mf {

// What a file-level call reports about the reads that pass (mf_report.cpp: reads per record, per group, k-mer depth).  Both ingest paths
// call after_pass once per mate batch right behind its filter pass, on the worker thread that ran the pass and on the read set that still
// holds the batch, and tally its pairs once the pair rule has decided which reads are kept.  Pairs are (read in the batch << 32) | record,
// the record being 0xFFFFFFFE for a passing read that no record wins; only passing reads have one.  A report that counts something else
// (depth) leaves the pairs empty and is made without counts: it tallies nothing.
struct PassReport {
    const uint32_t n_rec;
    // host pipeline: held[worker] = the read set that holds the batch the worker has just filtered (null: an empty batch), set by the
    // filter closure, which owns the read sets, and handed to after_pass by the same worker thread
    std::vector<mf_reads *> held;
    std::vector<uint64_t> counts;               // n_rec + 2: kept reads (mates one by one) assigned to each record, ambiguous, unassigned
    std::mutex mu;
    explicit PassReport(uint32_t n, bool tallies = true) : n_rec(n), counts(tallies ? (size_t)n + 2 : 0, 0) {}
    virtual ~PassReport() = default;
    virtual int after_pass(mf_reads *reads, std::vector<uint64_t> &pairs, std::string &err) = 0;
    // Right behind after_pass, on the same thread and read set: the host copy of that mate batch's pass bits (n reads), before the ingest
    // path stores them or the pair rule reads them.  A report that decides which mates are written clears bits here; the pair rule and
    // `kept` then work on what is left.  Most reports leave the bits alone.
    virtual int amend_bits(mf_reads *, uint32_t *, uint64_t, std::string &) { return 0; }
    virtual void restart() { counts.assign(counts.size(), 0); }          // the path that had taken the input declined it: nothing was kept
    // one mate's batch of n reads, n_kept of them kept (keep(i): read i is)
    template <class KeepFn> void add(const std::vector<uint64_t> &pairs, uint64_t n, uint64_t n_kept, KeepFn keep)
    {
        if (counts.empty()) return;
        std::lock_guard<std::mutex> lk(mu);
        uint64_t assigned = 0;
        for (const uint64_t pr : pairs) {
            const uint64_t i = pr >> 32; const uint32_t rec = (uint32_t)pr;
            if (i >= n || !keep(i)) continue;
            counts[rec < n_rec ? rec : n_rec]++; assigned++;
        }
        counts[(size_t)n_rec + 1] += n_kept - assigned;      // kept without passing themselves (a mate kept through its partner)
    }
};

// filter one packed mate batch on `device`; fills bits (ceil(n/32) u32).  Returns 0 or an MF_E_* code.
using BatchFilterFn = std::function<int(int device, const PackedHost &, uint64_t n, std::vector<uint32_t> &bits, std::string &err)>;

struct PipelineStats { uint64_t kept = 0, total = 0, batches = 0; };

int run_fastq_pipeline(const char *fq1, const char *fq2, const char *out1, const char *out2, bool pair_both,
                       int n_devices, int pack_threads, uint64_t batch_reads, const BatchFilterFn &filter,
                       PipelineStats &stats, std::string &err, PassReport *report = nullptr);

// ---------------------------------------------------------------- FASTQ quality filter (filter_v2)
struct QualParams {
    uint64_t start = 0, end = 0, ns = 10, trim = 0;
    uint32_t quality = 55; float limit = 0.2f;
    bool dedup = false, trunc = false;
};
bool utf8_valid(const char *p, size_t n);          // what Rust's `lines()` accepts (the reference unwraps header, sequence and quality line: main.rs:214-216, 287-289)
struct QualSpan { uint32_t s_off, s_len, q_off, q_len; };     // same layout as the kernels' QualRec
// counts of n records whose strings are offsets into text; with want_hashes the SipHash-1-3 values of the sequences are computed
// too and KEPT BY THE CALLEE for the dedup call that follows for the same records
using QualScanFn = std::function<int(const char *text, size_t len, const QualSpan *recs, uint32_t n, uint32_t quality,
                                     uint32_t *n_count, uint32_t *bad_count, bool want_hashes, std::string &err)>;
// de-duplication (main.rs:244-250) of the n records hashed by the last scan call, in file order over all calls: alive[i] = the record
// reached the dedup test; dup[i] = 1 when an earlier live record (of this or an earlier call) carried the same hash value
using QualDedupFn = std::function<int(const uint8_t *alive, uint32_t n, uint8_t *dup, std::string &err)>;
struct QualStats { uint64_t kept = 0, total = 0; bool panicked = false; };
// fq1 == nullptr: standard input; out2 == nullptr with fq2 set: standard output (reference: helper.rs:14-52)
int run_qualfilter_pipeline(const char *fq1, const char *fq2, const char *out1, const char *out2, const QualParams &p,
                            int threads, uint64_t batch_reads, const QualScanFn &scan, const QualDedupFn &dedup, QualStats &stats,
                            std::string &err);

} // namespace mf
