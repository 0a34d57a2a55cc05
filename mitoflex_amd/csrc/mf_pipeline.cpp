// The host side of both file-level calls, one translation unit: mf_pl_reader.h (channels, pools, BatchReader), mf_pl_stages.h (what the
// two pipelines share) and mf_qualdecide.h (the quality rules).  Each pipeline reads: context, readers, its middle stage, writers, join, timing.
#include "mf_pipeline.h"
#include "mf_pl_stages.h"

namespace mf {
struct PairBatch : ZipBatch { PackedHost packed[2]; };
using PairPtr = std::shared_ptr<PairBatch>;

int run_fastq_pipeline(const char *fq1, const char *fq2, const char *out1, const char *out2, bool pair_both,
                       int n_devices, int pack_threads, uint64_t batch_reads, const BatchFilterFn &filter,
                       PipelineStats &stats, std::string &err, PassReport *report)
{
    PipeRun run(fq1, fq2, out1, out2, err);
    const int nm = run.nm;
    std::atomic<uint64_t> t_pack{0}, t_dev{0};
    if (!run.open_readers(pack_threads / (2 * nm))) return MF_E_IO;

    // Batch buffers outlive the call (a handful of idle batches, about 1.5 GB for 2 M-record batches): giving a
    // gigabyte back to the kernel and faulting it in again costs 0.1 s per call, which matters to callers that
    // filter file after file (the bim loop).  MF_KEEP_BUFFERS=0 releases everything at the end of every call.
    static std::shared_ptr<Pool<MateBatch>> g_mate_pool = std::make_shared<Pool<MateBatch>>();
    static std::shared_ptr<Pool<PairBatch>> g_pair_pool = std::make_shared<Pool<PairBatch>>();
    const char *kb = getenv("MF_KEEP_BUFFERS"); const bool keep_buffers = !(kb && kb[0] == '0');
    auto mate_pool = keep_buffers ? g_mate_pool : std::make_shared<Pool<MateBatch>>();
    auto pair_pool = keep_buffers ? g_pair_pool : std::make_shared<Pool<PairBatch>>();
    std::vector<std::unique_ptr<Channel<PairPtr>>> q_dev;
    for (int d = 0; d < n_devices; d++) { q_dev.emplace_back(new Channel<PairPtr>(2)); run.watch(*q_dev.back()); }
    Channel<PairPtr> q_write[2] = {Channel<PairPtr>(4 * (size_t)n_devices + 4), Channel<PairPtr>(4 * (size_t)n_devices + 4)};
    for (auto &q : q_write) run.watch(q);
    run.start_readers(mate_pool, batch_reads);

    // ---- zip mates, pack, deal to devices (whole pairs stay together)
    run.threads.emplace_back([&] {
        MateZip zip{run.q_read, nm};
        for (uint64_t idx = 0;; idx++) {
            auto pb = pair_pool->get();
            if (!zip.next(*pb)) break;
            pb->index = idx;
            {
                ScopeTimer t{t_pack};
                if (nm == 2) {
                    std::thread t2([&] { pack_records(pb->recs(1), pb->n, pack_threads > 1 ? pack_threads / 2 : 1, pb->packed[1]); });
                    pack_records(pb->recs(0), pb->n, pack_threads > 1 ? pack_threads - pack_threads / 2 : 1, pb->packed[0]);
                    t2.join();
                } else pack_records(pb->recs(0), pb->n, pack_threads, pb->packed[0]);
            }
            if (!q_dev[idx % n_devices]->push(pb)) break;
        }
        run.stop_readers();
        for (auto &q : q_dev) q->finish();
    });

    // ---- one worker per device: H2D + kernels + D2H, then the pair rule
    std::mutex stat_mu; int dev_alive = n_devices;
    for (int d = 0; d < n_devices; d++)
        run.threads.emplace_back([&, d] {
            PairPtr pb;
            while (q_dev[d]->pop(pb)) {
                std::vector<uint32_t> bits[2]; std::vector<uint64_t> pairs[2];
                bool ok = true;
                for (int m = 0; m < nm && ok; m++) {
                    ScopeTimer t{t_dev};
                    std::string e;
                    int r = filter(d, pb->packed[m], pb->n, bits[m], e);
                    if (r == MF_OK && report) r = report->after_pass(report->held[d], pairs[m], e);      // (the worker's read set still holds this mate)
                    if (r == MF_OK && report) r = report->amend_bits(report->held[d], bits[m].data(), pb->n, e);
                    if (r != MF_OK) { run.fail(r, e); ok = false; }
                }
                if (!ok) break;
                pb->keep.assign(pb->n ? pb->n : 1, 0);
                uint64_t kc = 0;
                for (uint64_t i = 0; i < pb->n; i++) {
                    const int a = (bits[0][i >> 5] >> (i & 31)) & 1, b = nm == 2 ? (bits[1][i >> 5] >> (i & 31)) & 1 : 0;
                    const uint8_t k = (uint8_t)(nm == 2 ? (pair_both ? (a & b) : (a | b)) : a);
                    pb->keep[i] = k; kc += k;
                }
                if (report) for (int m = 0; m < nm; m++) report->add(pairs[m], pb->n, kc, [&](uint64_t i) { return pb->keep[i] != 0; });
                { std::lock_guard<std::mutex> lk(stat_mu); stats.kept += kc; stats.total += pb->n; stats.batches++; }
                for (int m = 0; m < nm; m++) if (!q_write[m].push(pb)) { ok = false; break; }
                if (!ok) break;
            }
            std::lock_guard<std::mutex> lk(stat_mu);
            if (--dev_alive == 0) for (int m = 0; m < nm; m++) q_write[m].finish();
        });
    for (int m = 0; m < nm; m++) run.threads.emplace_back([&, m] { write_records(run, m, q_write[m]); });
    run.join();
    const uint64_t t_joined = now_us();
    if (keep_buffers) { mate_pool->trim(8); pair_pool->trim(4); }   // every batch is back by now
    mate_pool.reset(); pair_pool.reset();                     // (not kept: the buffers are released here)
    if (run.timing)
        fprintf(stderr, "[mf pipeline] wall %.3f s (+%.3f s releasing buffers) | read %.3f %.3f | pack %.3f | device %.3f | write %.3f %.3f | batches %llu\n",
                (t_joined - run.t_start) / 1e6, (now_us() - t_joined) / 1e6, run.t_read[0] / 1e6, run.t_read[1] / 1e6, t_pack / 1e6, t_dev / 1e6, run.t_write[0] / 1e6, run.t_write[1] / 1e6,
                (unsigned long long)stats.batches);
    return run.rc;
}

// ================================================================ FASTQ quality filter (filter_v2)
// Same readers; the decision stage is one thread because the reference's -t budget is sequential (it stops at the first read
// that overflows it: filter/filter_bin/src/main.rs:254-259).  What is data parallel -- counting N and low-quality bytes,
// hashing the sequences, and the de-duplication set itself ("first occurrence wins" is a minimum over file indices, which needs
// no order of execution) -- runs on the GPU over the raw text of each batch.
bool utf8_valid(const char *p, size_t n)
{
    const unsigned char *s = (const unsigned char *)p; size_t i = 0;
    while (i < n) {
        if (i + 8 <= n) { uint64_t v; memcpy(&v, s + i, 8); if (!(v & 0x8080808080808080ULL)) { i += 8; continue; } }
        const unsigned char c = s[i];
        if (c < 0x80) { i++; continue; }
        int len; uint32_t cp, mn;
        if ((c & 0xE0) == 0xC0) { len = 2; cp = c & 0x1F; mn = 0x80; }
        else if ((c & 0xF0) == 0xE0) { len = 3; cp = c & 0x0F; mn = 0x800; }
        else if ((c & 0xF8) == 0xF0) { len = 4; cp = c & 0x07; mn = 0x10000; }
        else return false;
        if (i + len > n) return false;
        for (int k = 1; k < len; k++) { if ((s[i + k] & 0xC0) != 0x80) return false; cp = (cp << 6) | (s[i + k] & 0x3F); }
        if (cp < mn || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
        i += len;
    }
    return true;
}

using QualPtr = std::shared_ptr<ZipBatch>;
using SpanVec = std::vector<QualSpan, DefaultInitAlloc<QualSpan>>;
// GPU: the counts of one mate's first n records, their strings as offsets into the batch's text (and mate 1's hashes when de-duplicating)
static int scan_mate(const FqRec *recs, uint64_t n, int threads, uint32_t quality, bool want_hashes, const QualScanFn &scan, SpanVec &sp,
                     std::vector<uint32_t> &nc, std::vector<uint32_t> &bc, std::string &e)
{
    const char *base = recs[0].h, *endp = recs[n - 1].q + recs[n - 1].ql;
    if ((size_t)(endp - base) >= 0xFFFFFFF0ull) { e = "batch larger than 4 GiB: lower MF_BATCH_READS"; return MF_E_ARG; }
    sp.resize(n);
    parallel_chunks(n, threads, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) sp[i] = QualSpan{(uint32_t)(recs[i].s - base), recs[i].sl, (uint32_t)(recs[i].q - base), recs[i].ql};
    });
    nc.resize(n); bc.resize(n);
    return scan(base, (size_t)(endp - base), sp.data(), (uint32_t)n, quality, nc.data(), bc.data(), want_hashes, e);
}

int run_qualfilter_pipeline(const char *fq1, const char *fq2, const char *out1, const char *out2, const QualParams &P,
                            int threads, uint64_t batch_reads, const QualScanFn &scan, const QualDedupFn &dedup, QualStats &stats,
                            std::string &err)
{
    PipeRun run(fq1, fq2, out1, out2, err);
    const int nm = run.nm;
    std::atomic<uint64_t> t_check{0}, t_scan{0}, t_decide{0}, t_dedup{0}, t_wait_in{0}, t_wait_out{0};
    if (!run.open_readers(threads / (2 * nm))) return MF_E_IO;
    auto qual_pool = std::make_shared<Pool<ZipBatch>>();
    Channel<QualPtr> q_write[2] = {Channel<QualPtr>(4), Channel<QualPtr>(4)};
    for (auto &q : q_write) run.watch(q);
    run.start_readers(std::make_shared<Pool<MateBatch>>(), batch_reads);

    // ---- decisions (sequential semantics), GPU counting per batch: zip, check, scan, drop, dedup, take, push
    run.threads.emplace_back([&] {
        uint64_t budget = 0; bool stop = false;
        std::vector<uint32_t> nc[2], bc[2]; std::vector<uint8_t> alive, dupf; SpanVec sp;      // per-batch scratch, capacity kept
        MateZip zip{run.q_read, nm};
        for (uint64_t idx = 0; !stop; idx++) {
            auto qb = qual_pool->get();
            { ScopeTimer t{t_wait_in}; if (!zip.next(*qb)) break; }
            const uint64_t n = qb->n;
            FqRec *const mrec[2] = {qb->recs(0), nm == 2 ? qb->recs(1) : nullptr};
            uint64_t n_ok;
            { ScopeTimer t{t_check}; n_ok = qual_check_cut_batch(mrec, nm, n, P, threads); }
            if (!P.trunc && n_ok) {
                ScopeTimer t{t_scan};
                int r = MF_OK; std::string e;
                for (int m = 0; m < nm && r == MF_OK; m++) r = scan_mate(mrec[m], n_ok, threads, P.quality, m == 0 && P.dedup, scan, sp, nc[m], bc[m], e);
                if (r != MF_OK) { run.fail(r, e); break; }
            }
            {
                ScopeTimer t{t_decide};
                qb->keep.assign(n ? n : 1, 0);
                if (!P.trunc) {
                    alive.resize(n_ok ? n_ok : 1);
                    parallel_chunks(n_ok, threads, [&](uint64_t lo, uint64_t hi) {
                        for (uint64_t i = lo; i < hi; i++) {
                            const uint32_t ni[2] = {nc[0][i], nm == 2 ? nc[1][i] : 0}, bi[2] = {bc[0][i], nm == 2 ? bc[1][i] : 0};
                            alive[i] = !qual_drop(nm, mrec[0][i], ni, bi, P.ns, P.limit);
                        }
                    });
                    if (P.dedup && n_ok) {                                                                     // main.rs:244-250
                        dupf.resize(n_ok);
                        std::string e; int r;
                        { ScopeTimer td{t_dedup}; r = dedup(alive.data(), (uint32_t)n_ok, dupf.data(), e); }
                        if (r != MF_OK) { run.fail(r, e); break; }
                    }
                }
                const QualTake take = qual_take(P.trunc ? nullptr : alive.data(), !P.trunc && P.dedup ? dupf.data() : nullptr, mrec[0], n_ok, P.trim, budget, qb->keep.data());
                stats.kept += take.kept; stats.total += n_ok; stop = take.stop;
            }
            qb->n = n_ok; qb->index = idx;
            if (n_ok < n) { stats.panicked = true; stop = true; }
            ScopeTimer t{t_wait_out};
            for (int m = 0; m < nm; m++) if (!q_write[m].push(qb)) { stop = true; break; }
        }
        run.stop_readers();
        for (auto &q : q_write) q.finish();
    });
    for (int m = 0; m < nm; m++) run.threads.emplace_back([&, m] { write_records(run, m, q_write[m]); });
    run.join();
    if (run.timing)
        fprintf(stderr, "[mf qualfilter] wall %.3f s | read %.3f %.3f | decision thread: waiting for input %.3f, validate %.3f, scan (H2D, kernels, D2H) %.3f, decide %.3f (of which dedup on the device %.3f), waiting for the writers %.3f | write %.3f %.3f\n",
                (now_us() - run.t_start) / 1e6, run.t_read[0] / 1e6, run.t_read[1] / 1e6, t_wait_in / 1e6, t_check / 1e6, t_scan / 1e6, t_decide / 1e6, t_dedup / 1e6, t_wait_out / 1e6, run.t_write[0] / 1e6, run.t_write[1] / 1e6);
    return run.rc;
}

} // namespace mf
