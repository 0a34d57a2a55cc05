// Host pipeline, part 2 (see mf_pipeline.cpp): the stages both file-level pipelines are made of -- the run's context, the reader
// threads, the pairing of the two mates' batches, the ordered record writer, the scope timer.
#pragma once
#include "mf_pl_reader.h"
#include "mf_qualdecide.h"
#include "../../include/mitofilter.h"
#include <chrono>
#include <map>

namespace mf {
inline uint64_t now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// the time a scope takes, added to a stage's busy time (MF_PIPE_TIMING)
struct ScopeTimer {
    std::atomic<uint64_t> &acc; const uint64_t t0 = now_us();
    ~ScopeTimer() { acc += now_us() - t0; }
};
using MatePtr = std::shared_ptr<MateBatch>;
// What the zip hands on and the writers take: records first[m] .. first[m] + n - 1 of mate[m], and which of them are kept
struct ZipBatch {
    uint64_t index = 0, n = 0;
    MatePtr mate[2];
    uint64_t first[2] = {0, 0};
    std::vector<uint8_t> keep;
    void recycle() { mate[0].reset(); mate[1].reset(); keep.clear(); index = n = 0; first[0] = first[1] = 0; }
    FqRec *recs(int m) const { return mate[m]->recs.data() + first[m]; }
};

// ---- one run of a pipeline: the two readers and their channels, the first error, and every channel to abort when it is time to stop
struct PipeRun {
    const int nm;
    const char *in_path[2], *out_path[2];
    const bool timing = getenv("MF_PIPE_TIMING") != nullptr;      // busy seconds of every stage on stderr (diagnostics)
    const uint64_t t_start = now_us();
    std::atomic<uint64_t> t_read[2] = {{0}, {0}}, t_write[2] = {{0}, {0}};
    BatchReader rd[2];
    // set with the channels' abort and when the middle stage stops (budget spent, panic, short mate file, error): the readers stop reading ahead
    std::atomic<bool> winding_down{false};
    Channel<MatePtr> q_read[2] = {Channel<MatePtr>(2), Channel<MatePtr>(2)};
    std::vector<std::thread> threads;
    int rc = MF_OK;
    PipeRun(const char *fq1, const char *fq2, const char *out1, const char *out2, std::string &err)
        : nm(fq2 ? 2 : 1), in_path{fq1, fq2}, out_path{out1, out2}, err_(err) { watch(q_read[0]); watch(q_read[1]); }
    bool open_readers(int parse_threads)                    // (plain files: segments parsed in parallel)
    {
        for (int m = 0; m < nm; m++) { rd[m].set_stop_flag(&winding_down); rd[m].set_parse_threads(parse_threads); if (!rd[m].open(in_path[m], err_)) return false; }
        return true;
    }
    void watch(ChannelBase &c) { channels_.push_back(&c); }
    void set_err(int code, const std::string &msg) { std::lock_guard<std::mutex> lk(err_mu_); if (rc == MF_OK) { rc = code; err_ = msg; } }      // the first error wins
    void abort_all() { winding_down = true; for (ChannelBase *c : channels_) c->abort(); }
    void fail(int code, const std::string &msg) { set_err(code, msg); abort_all(); }
    void stop_readers() { winding_down = true; for (auto &q : q_read) q.abort(); }      // (they may still be producing past the end of the shorter file)
    void start_readers(std::shared_ptr<Pool<MateBatch>> pool, uint64_t batch_reads)
    {
        for (int m = 0; m < nm; m++)
            threads.emplace_back([this, m, pool, batch_reads] {
                for (;;) {
                    auto b = pool->get();
                    std::string e;
                    bool got;
                    { ScopeTimer t{t_read[m]}; got = rd[m].next(*b, batch_reads, e); }
                    if (!got) { if (!e.empty()) fail(MF_E_IO, e); break; }
                    if (!q_read[m].push(b)) break;
                }
                q_read[m].finish();
            });
    }
    void join() { for (auto &t : threads) t.join(); }
private:
    std::mutex err_mu_; std::string &err_; std::vector<ChannelBase *> channels_;
};

// ---- the two read channels as one sequence of pair batches.  Mates are paired BY RECORD COUNT: the batches of the two readers need
// not be of equal size (a pipe whose producer pauses hands over what it has), so what is left of the longer batch is paired with the
// other mate's next one.  A mate has run out only when its reader has (zip semantics: the shorter file bounds the pair count,
// filter/filter_bin/src/main.rs:214).
struct MateZip {
    Channel<MatePtr> *q_; const int nm_;                    // the two read channels; one mate or two
    MatePtr cur_[2] = {}; uint64_t pos_[2] = {0, 0};
    // fills b.n, b.mate and b.first; false: a reader has run out (or the channels were aborted)
    bool next(ZipBatch &b)
    {
        for (int m = 0; m < nm_; m++)
            while (!cur_[m] || pos_[m] == cur_[m]->recs.size()) { cur_[m].reset(); pos_[m] = 0; if (!q_[m].pop(cur_[m])) return false; }
        b.n = cur_[0]->recs.size() - pos_[0];
        if (nm_ == 2 && cur_[1]->recs.size() - pos_[1] < b.n) b.n = cur_[1]->recs.size() - pos_[1];
        for (int m = 0; m < nm_; m++) { b.mate[m] = cur_[m]; b.first[m] = pos_[m]; pos_[m] += b.n; }
        return true;
    }
};

// ---- the writer of output file m (null: standard output): the kept records of every batch as header / seq / "+" / qual (filter_bin
// main.rs:261-268, 317-321), in the order of the batches' indices (device workers may finish out of order)
template <class B> void write_records(PipeRun &run, int m, Channel<std::shared_ptr<B>> &q)
{
    const char *name = run.out_path[m] ? run.out_path[m] : "<stdout>";
    OutFile of;
    if (!of.open(run.out_path[m])) { run.fail(MF_E_IO, std::string("Cannot open file ") + name); return; }
    std::map<uint64_t, std::shared_ptr<B>> pending; uint64_t next = 0; bool ok = true;
    std::vector<char> buf; buf.reserve((1u << 22) + (1u << 16));
    auto drain = [&] { if (!buf.empty() && !of.write(buf.data(), buf.size())) ok = false; buf.clear(); };
    std::shared_ptr<B> pb;
    while (ok && q.pop(pb)) {
        pending[pb->index] = pb;
        while (ok && !pending.empty() && pending.begin()->first == next) {
            ScopeTimer t{run.t_write[m]};
            std::shared_ptr<B> cur = pending.begin()->second; pending.erase(pending.begin()); next++;
            const FqRec *recs = cur->recs(m);
            for (uint64_t i = 0; i < cur->n && ok; i++) {
                if (!cur->keep[i]) continue;
                const FqRec &r = recs[i];
                buf.insert(buf.end(), r.h, r.h + r.hl); buf.push_back('\n');
                buf.insert(buf.end(), r.s, r.s + r.sl); buf.push_back('\n'); buf.push_back('+'); buf.push_back('\n');
                buf.insert(buf.end(), r.q, r.q + r.ql); buf.push_back('\n');
                if (buf.size() > (1u << 22)) drain();
            }
        }
    }
    drain();
    ok = of.close() && ok;
    if (!ok) run.fail(MF_E_IO, std::string("write error on ") + name);
}

// ---- fn(lo, hi) over [0, n) cut into one contiguous chunk per worker
template <class F> void parallel_chunks(uint64_t n, int threads, F fn)
{
    if (threads < 1) threads = 1;
    if ((uint64_t)threads > n / 4096 + 1) threads = (int)(n / 4096 + 1);      // not worth a thread below a few thousand records
    if (threads == 1) { fn((uint64_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 1; t < threads; t++) th.emplace_back(fn, n * (uint64_t)t / threads, n * (uint64_t)(t + 1) / threads);
    fn((uint64_t)0, n / threads);
    for (auto &x : th) x.join();
}

// qual_check_cut over a batch cut into chunks (records are independent there): each chunk stops at its first offender and the earliest
// one bounds the batch (records past it are never looked at again).  Returns its index, or n.
inline uint64_t qual_check_cut_batch(FqRec *const mrec[2], int nm, uint64_t n, const QualParams &P, int threads)
{
    std::atomic<uint64_t> first_bad{n};
    parallel_chunks(n, threads, [&](uint64_t lo, uint64_t hi) {
        const uint64_t i = qual_check_cut(mrec, nm, lo, hi, P);
        uint64_t cur = first_bad.load();
        while (i < hi && i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
    });
    return first_bad.load();
}

} // namespace mf
