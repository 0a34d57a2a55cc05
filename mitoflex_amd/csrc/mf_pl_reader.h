// Host pipeline, part 1 (see mf_pipeline.cpp): bounded channels, batch pools and the batched FASTQ reader.
#pragma once
#include "mf_host.h"
#include "mf_inflate.h"
#include "mf_pinflate.h"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <poll.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <thread>
#include <zlib.h>

namespace mf {
// -------------------------------------------------------------- bounded channel
// (the base is what does not depend on the payload: a pipeline run keeps its channels by it to abort them all at once)
class ChannelBase {
public:
    void finish() { std::lock_guard<std::mutex> lk(mu_); done_ = true; cv_item_.notify_all(); }          // no more items
    void abort() { std::lock_guard<std::mutex> lk(mu_); closed_ = true; cv_item_.notify_all(); cv_space_.notify_all(); }
protected:
    std::mutex mu_; std::condition_variable cv_item_, cv_space_; bool done_ = false, closed_ = false;
};
template <class T> class Channel : public ChannelBase {
public:
    explicit Channel(size_t cap) : cap_(cap) {}
    bool push(T v)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_space_.wait(lk, [&] { return q_.size() < cap_ || closed_; });
        if (closed_) return false;
        q_.push_back(std::move(v));
        cv_item_.notify_one();
        return true;
    }
    bool pop(T &v)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_item_.wait(lk, [&] { return !q_.empty() || done_ || closed_; });
        if (closed_ || q_.empty()) return false;
        v = std::move(q_.front()); q_.pop_front();
        cv_space_.notify_one();
        return true;
    }
private:
    std::deque<T> q_; size_t cap_;
};

// --------------------------------------------------------- batched FASTQ reader
// Hands out batches of up to `max_records` complete 4-line records.  The reference's conventions
// apply to the stream as a whole (filter/filter_bin/src/main.rs:287-321): a partial record at the
// very end is dropped, CR before LF is stripped.
// text is a malloc'd buffer (no zero fill on growth); recs point into it
struct MappedFile {                       // a plain input file mapped read-only for the run
    const char *p = nullptr; size_t n = 0;
    ~MappedFile() { if (p) munmap(const_cast<char *>(p), n); }
};

// Batch objects are recycled through a pool: their vectors keep their capacity, so a steady-state batch
// touches no freshly mapped memory (page faults on new mappings serialise on the process's mmap lock and
// were the limit of the pack and parse stages with many threads).
template <class T> class Pool : public std::enable_shared_from_this<Pool<T>> {
public:
    std::shared_ptr<T> get()
    {
        T *p = nullptr;
        { std::lock_guard<std::mutex> lk(mu_); if (!free_.empty()) { p = free_.back().release(); free_.pop_back(); } }
        if (!p) p = new T();
        auto self = this->shared_from_this();
        return std::shared_ptr<T>(p, [self](T *x) { x->recycle(); std::lock_guard<std::mutex> lk(self->mu_); self->free_.emplace_back(x); });
    }
    // keep at most `keep` idle objects (the rest is released)
    void trim(size_t keep) { std::lock_guard<std::mutex> lk(mu_); while (free_.size() > keep) free_.pop_back(); }
private:
    std::mutex mu_; std::vector<std::unique_ptr<T>> free_;
};

using RecVec = std::vector<FqRec, DefaultInitAlloc<FqRec>>;
struct MateBatch {
    char *text = nullptr; size_t len = 0, cap = 0;
    RecVec recs;
    std::shared_ptr<MappedFile> map;      // set when recs point into a mapped file instead of `text`
    ~MateBatch() { free(text); }
    void recycle() { recs.clear(); len = 0; map.reset(); }
    // the text buffer of a stream-mode batch (hundreds of MB): 2 MiB aligned and marked for huge pages, like the vectors
    bool reserve(size_t want)
    {
        if (want <= cap) return true;
        size_t nc = cap ? cap : ((size_t)64 << 20);
        while (nc < want) nc *= 2;
        const size_t huge = (size_t)2 << 20;
        nc = (nc + huge - 1) / huge * huge;
        char *p = (char *)aligned_alloc(huge, nc);
        if (!p) return false;
        madvise(p, nc, MADV_HUGEPAGE);
        if (len) memcpy(p, text, len);
        free(text);
        text = p; cap = nc;
        return true;
    }
};

class BatchReader {
public:
    // a regular .gz file mapped for the library's decoders, or a gzopen / fopen stream, or on top of that a regular plain file mapped
    bool open(const char *path, std::string &err)
    {
        if (!path) { f_ = stdin; own_f_ = false; path_ = "<stdin>"; return true; }
        path_ = path;
        gz_ = has_gz_ext(path);
        if (gz_ && !getenv("MF_ZLIB_INFLATE") && open_gz_mapped(path)) return true;
        if (gz_) { g_ = gzopen(path, "rb"); if (g_) gzbuffer(g_, 1 << 20); }
        else f_ = fopen(path, "rb");
        if (!g_ && !f_) { err = std::string("Cannot open file ") + path; return false; }
        if (f_) setvbuf(f_, nullptr, _IONBF, 0);             // we read in 16 MiB blocks ourselves
        if (f_ && parse_threads_ > 1) map_ = map_regular(fileno(f_), false);
        return true;
    }
    void set_parse_threads(int t) { parse_threads_ = t < 1 ? 1 : t; }
    void set_stop_flag(const std::atomic<bool> *f) { stop_ = f; }
    ~BatchReader() { if (g_) gzclose(g_); if (f_ && own_f_) fclose(f_); }
    // false at end of stream (no records left) or on error (err set)
    bool next(MateBatch &b, uint64_t max_records, std::string &err)
    {
        if (map_) return next_mapped(b, max_records);
        if (parse_threads_ > 1 && !serial_parse_) return next_stream_indexed(b, max_records, err);
        return next_stream_serial(b, max_records, err);
    }
private:
    // the regular file behind fd, mapped read-only (an empty one, where that is accepted, maps to nothing); null: not regular, or no mapping
    static std::shared_ptr<MappedFile> map_regular(int fd, bool empty_ok)
    {
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || (st.st_size == 0 && !empty_ok)) return nullptr;
        auto mf = std::make_shared<MappedFile>();
        if (st.st_size == 0) return mf;
        void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return nullptr;
        mf->p = (const char *)m; mf->n = (size_t)st.st_size; madvise(m, mf->n, MADV_SEQUENTIAL);
        return mf;
    }
    // regular .gz file: map it and decode with the streaming decoder; false: the zlib stream takes it
    bool open_gz_mapped(const char *path)
    {
        const int fd = ::open(path, O_RDONLY);
        gzmap_ = map_regular(fd, true);
        if (fd >= 0) ::close(fd);
        if (!gzmap_) return false;
        // big files: several chunks of the one stream are decoded at a time (mf_pinflate.h)
        par_gz_ = parse_threads_ >= 3 && gzmap_->n >= ((size_t)16 << 20) && !getenv("MF_SERIAL_INFLATE");
        if (par_gz_) pinflater_.open((const uint8_t *)gzmap_->p, gzmap_->n, parse_threads_);
        else inflater_.open((const uint8_t *)gzmap_->p, gzmap_->n);
        return true;
    }
    // ---- the carry-over of the stream modes: what lies behind a batch's last record opens the next batch
    bool start_batch(MateBatch &b, std::string &err)
    {
        b.recs.clear(); b.len = 0;
        if (carry_.empty()) return true;
        if (!b.reserve(carry_.size())) { err = "out of memory"; return false; }
        memcpy(b.text, carry_.data(), carry_.size()); b.len = carry_.size(); carry_.clear();
        return true;
    }
    void carry_from(MateBatch &b, size_t cut) { carry_.assign(b.text + cut, b.text + b.len); b.len = cut; }
    // ---- stream mode on one thread.  One pass: bytes are read in blocks and lines are cut as they arrive; every fourth line closes a
    // record.  Record fields are kept as offsets while the buffer may still move, pointers afterwards.
    bool next_stream_serial(MateBatch &b, uint64_t max_records, std::string &err)
    {
        if (!start_batch(b, err)) return false;
        struct Off { size_t h, s, q; uint32_t hl, sl, ql; };
        std::vector<Off> off; off.reserve(max_records < (1u << 22) ? max_records : (1u << 22));
        size_t pos = 0, line_start = 0; int li = 0; size_t ls[4]; uint32_t ll[4]; size_t cut = 0, rec_end = 0; bool full = false, short_read = false;
        const size_t blk = 16u << 20;
        for (;;) {
            while (pos < b.len) {
                const char *nl = (const char *)memchr(b.text + pos, '\n', b.len - pos);
                if (!nl) { pos = b.len; break; }
                size_t e = (size_t)(nl - b.text), L = e - line_start;
                if (L && b.text[e - 1] == '\r') L--;          // lines() strips "\r\n"
                ls[li] = line_start; ll[li] = (uint32_t)L;
                line_start = pos = e + 1;
                if (++li == 4) {
                    li = 0;
                    off.push_back(Off{ls[0], ls[1], ls[3], ll[0], ll[1], ll[3]});
                    rec_end = pos;
                    if (off.size() == max_records) { cut = pos; full = true; break; }
                }
            }
            if (full || eof_) break;
            // a pipe or stdin whose producer has had nothing more for a while: hand over the complete records (see read_some)
            if (short_read && !off.empty()) { cut = rec_end; full = true; break; }
            if (!fill(b, blk, err)) return false;
            short_read = idle_;
        }
        if (full) carry_from(b, cut);
        else if (eof_ && li == 3 && line_start < b.len) {
            // the stream ended inside the 4th line of a record without a final LF: lines() still yields it
            size_t L = b.len - line_start; if (L && b.text[b.len - 1] == '\r') L--;
            off.push_back(Off{ls[0], ls[1], line_start, ll[0], ll[1], (uint32_t)L});
        }
        b.recs.resize(off.size());
        for (size_t i = 0; i < off.size(); i++)
            b.recs[i] = FqRec{b.text + off[i].h, b.text + off[i].s, b.text + off[i].q, off[i].hl, off[i].sl, off[i].ql};
        return !b.recs.empty();
    }
    // ---- indexed parsing of a text buffer (a mapped plain file, or the decoded text of a stream batch).
    // The buffer is cut into segments of SEG bytes.  Newlines are counted per segment in parallel; a
    // prefix sum gives every segment the index of the first line that starts in it, hence the index of
    // the first record whose header starts in it.  A range of record indices is then parsed by the
    // segments holding those headers, in parallel, every record written straight to its slot (a record
    // is followed across the segment border).
    size_t SEG = getenv("MF_PARSE_SEG") ? (size_t)strtoull(getenv("MF_PARSE_SEG"), nullptr, 10) : (size_t)(4u << 20);   // bytes per parse segment
    const bool serial_parse_ = getenv("MF_SERIAL_PARSE") != nullptr;      // streams are cut on one thread whatever parse_threads_ is
    struct LineIndex { std::vector<uint64_t> first_line; uint64_t n_records = 0; };
    // final: the buffer ends where the input ends, so an unterminated last line is a line (lines() yields it)
    void build_index(const char *p, size_t n, bool final, LineIndex &ix)
    {
        const size_t nseg = (n + SEG - 1) / SEG;
        std::vector<uint64_t> cnt(nseg, 0);
        parallel_for(nseg, [&](size_t i) {
            const char *q = p + i * SEG, *e = p + std::min(n, (i + 1) * SEG); uint64_t c = 0;
            while (q < e) { const char *nl = (const char *)memchr(q, '\n', (size_t)(e - q)); if (!nl) break; c++; q = nl + 1; }
            cnt[i] = c;
        });
        // first_line[i]: index of the first line that STARTS inside segment i (a line starts after every '\n' and at 0)
        ix.first_line.assign(nseg + 1, 0);
        uint64_t newlines = 0;
        for (size_t i = 0; i < nseg; i++) {
            const size_t off = i * SEG;
            ix.first_line[i] = newlines + ((off > 0 && p[off - 1] != '\n') ? 1 : 0);
            newlines += cnt[i];
        }
        const uint64_t total_lines = newlines + ((final && n > 0 && p[n - 1] != '\n') ? 1 : 0);
        ix.first_line[nseg] = total_lines;
        ix.n_records = total_lines / 4;                     // a partial record at the very end is dropped / left for the next batch
    }
    // records [r0, r1) of the buffer -> out[0 .. r1-r0); *end_off (optional): offset just behind record r1-1
    void parse_records(const char *p, size_t n, const LineIndex &ix, uint64_t r0, uint64_t r1, FqRec *out, size_t *end_off)
    {
        const size_t nseg = (n + SEG - 1) / SEG;
        auto rec_base = [&](size_t i) { return (ix.first_line[i] + 3) / 4; };      // records whose header starts in segments before i
        // first segment holding record r0's header: the last i with rec_base(i) <= r0
        size_t lo = 0, hi = nseg;
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (rec_base(mid) <= r0) lo = mid; else hi = mid; }
        size_t s0 = lo, s1 = s0;
        while (s1 < nseg && rec_base(s1) < r1) s1++;
        parallel_for(s1 - s0, [&](size_t gi) {
            const size_t i = s0 + gi, off = i * SEG, end = std::min(n, off + SEG);
            uint64_t line = ix.first_line[i];
            size_t pos = off;
            if (off > 0 && p[off - 1] != '\n') {            // byte `off` continues an earlier line
                const char *nl = (const char *)memchr(p + off, '\n', n - off);
                if (!nl) return;
                pos = (size_t)(nl - p) + 1;
            }
            // skip to the next header line (index divisible by 4)
            while (pos < n && (line & 3)) {
                const char *nl = (const char *)memchr(p + pos, '\n', n - pos);
                if (!nl) return;
                pos = (size_t)(nl - p) + 1; line++;
            }
            uint64_t rec = line / 4;
            while (pos < end && rec < r1) {                 // this record's header starts inside the segment
                const char *ls[4]; uint32_t ll[4]; int li = 0;
                size_t q = pos;
                for (; li < 4 && q < n; li++) {
                    const char *nl = (const char *)memchr(p + q, '\n', n - q);
                    const size_t e = nl ? (size_t)(nl - p) : n;
                    size_t L = e - q; if (L && p[e - 1] == '\r') L--;      // lines() strips "\r\n"
                    ls[li] = p + q; ll[li] = (uint32_t)L;
                    if (!nl) { q = n; li++; break; }
                    q = e + 1;
                }
                if (li < 4) break;                          // partial record at the very end
                if (rec >= r0) out[rec - r0] = FqRec{ls[0], ls[1], ls[3], ll[0], ll[1], ll[3]};
                if (rec + 1 == r1 && end_off) *end_off = q;
                rec++;
                pos = q;
            }
        });
    }
    // ---- mapped mode: the whole file is indexed once, a batch is a range of record indices
    bool next_mapped(MateBatch &b, uint64_t max_records)
    {
        b.recs.clear(); b.map = map_;
        if (!indexed_) { build_index(map_->p, map_->n, true, map_ix_); indexed_ = true; }
        if (rec_pos_ >= map_ix_.n_records) return false;
        const uint64_t r0 = rec_pos_, r1 = std::min<uint64_t>(map_ix_.n_records, r0 + max_records);
        b.recs.resize((size_t)(r1 - r0));
        parse_records(map_->p, map_->n, map_ix_, r0, r1, b.recs.data(), nullptr);
        rec_pos_ = r1;
        return true;
    }
    // one read of up to `want` bytes behind the batch's text (none: the stream has ended); false: asked to stop, or an error (err set)
    bool fill(MateBatch &b, size_t want, std::string &err)
    {
        if (stopped()) return false;
        if (!b.reserve(b.len + want)) { err = "out of memory"; return false; }
        idle_ = false;
        const long got = read_some(b.text + b.len, want, err);
        if (got < 0) return false;
        if (got == 0) eof_ = true; else b.len += (size_t)got;
        return true;
    }
    long read_some(char *dst, size_t want, std::string &err)          // bytes read, or -1
    {
        if (gzmap_) {
            std::string why;
            const long n = par_gz_ ? pinflater_.read((uint8_t *)dst, want, why) : inflater_.read((uint8_t *)dst, want, why);
            if (n < 0) err = "gzip read error in " + path_ + ": " + why;
            return n;
        }
        if (gz_) { const int n = gzread(g_, dst, (unsigned)std::min<size_t>(want, (size_t)1 << 30)); if (n < 0) err = "gzip read error in " + path_; return n; }
        // plain stream (pipe, stdin; the stream is unbuffered).  A pipe hands over at most 64 KiB per read(): keep reading until the
        // block is full, so that batch boundaries do not depend on how the producer's writes happen to arrive -- but if the
        // producer has had nothing for 50 ms, return what is there (idle_ set): the reference works line by line, and with a -t
        // budget it may never need the rest of a slow stream.  The poll also lets the stop flag be seen in good time.
        long total = 0;
        for (;;) {
            struct pollfd pfd; pfd.fd = fileno(f_); pfd.events = POLLIN; pfd.revents = 0;
            const int pr = poll(&pfd, 1, 50);                 // a blocked read() cannot be told to stop; a poll that times out can
            if (stopped()) return -1;                                 // (no error text: the pipeline is winding down for its own reasons)
            if (pr == 0) { if (total) { idle_ = true; return total; } continue; }
            const ssize_t n = ::read(fileno(f_), dst + total, want - (size_t)total);
            if (n > 0) { total += n; if ((size_t)total == want) return total; continue; }
            if (n == 0) return total;                         // end of the stream (the next call returns 0)
            if (errno != EINTR && errno != EAGAIN) { err = "read error in " + path_; return -1; }
        }
    }
    // the pipeline is winding down (error elsewhere, the -t budget is spent, a mate file ran out): stop reading ahead
    bool stopped() const { return stop_ && stop_->load(std::memory_order_relaxed); }
    // ---- stream mode with several threads (decoded .gz text, pipes): enough text for the batch is read
    // first, then indexed and parsed like a mapped file; what lies behind the last record goes to the next batch
    bool next_stream_indexed(MateBatch &b, uint64_t max_records, std::string &err)
    {
        if (!start_batch(b, err)) return false;
        LineIndex ix;
        size_t target = (size_t)((double)max_records * rec_bytes_est_ * 1.02) + 4096;
        const bool live = !gz_ && !gzmap_;                 // a pipe or stdin: the producer may be slower than we are
        for (;;) {
            bool short_read = false;
            while (!eof_ && b.len < target) {
                if (!fill(b, std::min<size_t>((size_t)64 << 20, std::max<size_t>((size_t)1 << 16, target - b.len)), err)) return false;
                // the producer has had nothing more for a while: hand over the records that are complete instead of waiting for a
                // whole batch (the reference works line by line -- with a -t budget it may never need the rest)
                if (live && idle_) { short_read = true; break; }
            }
            build_index(b.text, b.len, eof_, ix);
            if (ix.n_records >= max_records || eof_ || (short_read && ix.n_records > 0)) break;
            const double per = ix.n_records ? (double)b.len / (double)ix.n_records : rec_bytes_est_ * 2;
            target = b.len + (size_t)((double)(max_records - ix.n_records + 1) * per * 1.05) + ((size_t)1 << 16);
        }
        const uint64_t take = std::min<uint64_t>(max_records, ix.n_records);
        if (take == 0) return false;                        // nothing but a partial record left: dropped
        b.recs.resize((size_t)take);
        size_t cut = b.len;
        parse_records(b.text, b.len, ix, 0, take, b.recs.data(), &cut);
        rec_bytes_est_ = 0.5 * rec_bytes_est_ + 0.5 * ((double)cut / (double)take);
        if (take < ix.n_records || !eof_) carry_from(b, cut); else b.len = cut;
        return true;
    }
    template <class F> void parallel_for(size_t count, F f)
    {
        std::vector<std::thread> th;
        const size_t T = std::min<size_t>(count, (size_t)parse_threads_);
        std::atomic<size_t> nexti{0};
        for (size_t t = 1; t < T; t++) th.emplace_back([&] { for (size_t i; (i = nexti++) < count;) f(i); });
        for (size_t i; (i = nexti++) < count;) f(i);
        for (auto &x : th) x.join();
    }
    bool gz_ = false, eof_ = false, own_f_ = true; gzFile g_ = nullptr; FILE *f_ = nullptr; std::string path_;
    std::shared_ptr<MappedFile> gzmap_; GzInflater inflater_;   // .gz input: the compressed file, mapped, and its decoder
    ParallelGzReader pinflater_; bool par_gz_ = false;
    std::vector<char> carry_;
    int parse_threads_ = 1;
    const std::atomic<bool> *stop_ = nullptr;
    std::shared_ptr<MappedFile> map_;
    LineIndex map_ix_; bool indexed_ = false;
    uint64_t rec_pos_ = 0;
    double rec_bytes_est_ = 350.0;                      // bytes per record seen so far (stream mode read-ahead)
    bool idle_ = false;                                 // read_some returned early because a live producer had nothing for a while
};

} // namespace mf
