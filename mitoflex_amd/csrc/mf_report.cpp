// libmitofilter_hip: the reports on the reads that pass the filter -- reads per bait record (mf_assign), per group of records
// (mf_assign_groups), k-mer depth along the records (mf_depth), position, strand and base depth (mf_place), base counts, consensus and
// variants (mf_pileup), per-read mismatches and an identity cut on the placed reads (mf_verify) -- and their file-level calls.
// Each runs behind a filter pass of mf_api.cpp on the read set that still holds the pass's bitmap; the kernels are mf_assign.hip's and
// mf_place.hip's.
#include "mf_api_internal.h"
#include "mf_pipeline.h"
#include "mf_align.h"
#include "mf_pairs.h"

#include <atomic>
#include <string.h>

using namespace mf;

// record j holds positions [starts[j], starts[j + 1]) of the set (bases or residues): n_rec + 1 offsets
static std::vector<uint64_t> record_starts(const mf_kmerset *ks)
{
    const std::vector<uint64_t> &len = ks->rec_len();
    std::vector<uint64_t> starts(len.size() + 1, 0);
    for (size_t j = 0; j < len.size(); j++) starts[j + 1] = starts[j] + len[j];
    return starts;
}

// A set's bait on the device for the time of a table build: bases (nucleotide) or residues (protein), run lengths, record starts.
// Released with the build's other temporaries (tmp) on every exit path.
struct BaitOnDevice {
    DevScratch tmp;
    BaitView view{nullptr, 0, nullptr};          // words: null for a protein set
    const uint8_t *aa = nullptr;                 // residues: null for a nucleotide set
    const uint64_t *rec_start = nullptr; uint32_t n_rec = 0;
    std::vector<uint64_t> starts;                // (the host copy lives as long as the upload may be running)
    template <class T> int put(const T *&d, const std::vector<T> &h, hipStream_t st)
    {
        T *p = nullptr;
        HIPCHK(tmp.alloc(p, h.size() * sizeof(T)));
        HIPCHK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
        d = p;
        return MF_OK;
    }
    int upload(const mf_kmerset *ks, hipStream_t st)
    {
        const bool prot = ks->kind == MF_KIND_PROTEIN;
        starts = record_starts(ks);
        n_rec = (uint32_t)starts.size() - 1;
        view.total = ks->positions();
        int rc = prot ? put(aa, ks->pbait.aa, st) : put(view.words, ks->bait.words, st);
        if (rc == MF_OK) rc = put(view.runlen, prot ? ks->pbait.runlen : ks->bait.runlen, st);
        if (rc == MF_OK) rc = put(rec_start, starts, st);
        return rc;
    }
};

// -------------------------------------------------------- record and group assignment
// The owner table of a set on `device` (its tables are built) in `slot`: T->owner, by record (what mf_assign uses, whatever the set's
// grouping), or T->gowner with the set's record -> group map, for its current grouping (mf_kmerset_group_records frees it).  Made by the
// first call that asks for it, under the set's lock; sets that never assign reads never hold one.
static int owner_table(mf_kmerset *ks, int device, const DevTables *T, uint32_t *&slot, const std::vector<uint32_t> *rec_group)
{
    std::lock_guard<std::mutex> lk(ks->mu);
    if (slot) return MF_OK;
    DevCtx *ctx; int rc = get_ctx(device, &ctx); if (rc) return rc;
    hipStream_t st = ctx->stream;
    BaitOnDevice B;
    rc = B.upload(ks, st); if (rc) return rc;
    const uint32_t *d_group = nullptr; uint32_t *d_hi = nullptr, *owner = nullptr;
    if (rec_group && !rec_group->empty()) { rc = B.put(d_group, *rec_group, st); if (rc) return rc; }
    HIPCHK(B.tmp.alloc(d_hi, ks->slots * 4));
    HIPCHK(B.tmp.alloc(owner, ks->slots * 4));
    HIPCHK(B.aa ? launch_build_powner(B.aa, B.view.runlen, B.view.total, B.rec_start, B.n_rec, d_group, T->view, owner, d_hi, st)
                : launch_build_owner(B.view, B.rec_start, B.n_rec, d_group, T->view, owner, d_hi, st));
    HIPCHK(hipStreamSynchronize(st));
    slot = B.tmp.release(owner);
    return MF_OK;
}

// Assignment of the reads that passed the filter pass just run on this read set (its bitmap in r->d_bits[r->cur]).  assign_out: n_reads words;
// record_reads: n_rec + 2 counts; pairs: (read << 32) | record of every passing read, in no particular order.  Each optional.
// by_group: to the set's groups instead of its records (the group-owner table; n_rec is then the number of groups).
static int assign_after_filter(mf_kmerset *ks, mf_reads *r, uint32_t *assign_out, uint64_t *record_reads, std::vector<uint64_t> *pairs, bool by_group)
{
    DevTables *T; int rc = build_on_device(ks, r->device, &T); if (rc) return rc;
    rc = by_group ? owner_table(ks, r->device, T, T->gowner, &ks->rec_group) : owner_table(ks, r->device, T, T->owner, nullptr); if (rc) return rc;
    const uint32_t *owner = by_group ? T->gowner : T->owner;
    DevCtx *ctx; rc = get_ctx(r->device, &ctx, r->lane); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n = r->v.n_reads;
    const uint32_t n_rec = by_group ? ks->n_groups() : (uint32_t)ks->bait.rec_len.size();
    const size_t n_cnt = (size_t)n_rec + 2;                          // records, ambiguous, the length of the list
    HIPCHK(dev_reserve(r->d_acnt, r->cap_acnt, n_cnt * 8, false));
    HIPCHK(hipMemsetAsync(r->d_acnt, 0, n_cnt * 8, st));
    if (n) {
        HIPCHK(dev_reserve(r->d_alist, r->cap_alist, n * 4, true));
        if (assign_out) { HIPCHK(dev_reserve(r->d_assign, r->cap_assign, n * 4, true)); HIPCHK(hipMemsetAsync(r->d_assign, 0xFF, n * 4, st)); }
        if (pairs) HIPCHK(dev_reserve(r->d_apairs, r->cap_apairs, n * 8, true));
        HIPCHK(launch_pass_list(r->d_bits[r->cur], n, r->d_alist, r->d_acnt + n_rec + 1, st));
        HIPCHK(launch_assign(r->v, T->view, owner, r->d_alist, r->d_acnt + n_rec + 1, n_rec, assign_out ? r->d_assign : nullptr,
                             pairs ? r->d_apairs : nullptr, r->d_acnt, ctx->n_cu, st));
    }
    std::vector<unsigned long long> cnt(n_cnt, 0);
    HIPCHK(hipMemcpyAsync(cnt.data(), r->d_acnt, n_cnt * 8, hipMemcpyDeviceToHost, st));
    if (assign_out && n) HIPCHK(hipMemcpyAsync(assign_out, r->d_assign, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t listed = cnt[n_rec + 1];
    if (pairs) {
        pairs->resize(listed);
        if (listed) { HIPCHK(hipMemcpyAsync(pairs->data(), r->d_apairs, listed * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); }
    }
    if (record_reads) {
        for (uint32_t j = 0; j <= n_rec; j++) record_reads[j] = cnt[j];
        record_reads[n_rec + 1] = n - listed;
    }
    return MF_OK;
}

static int need_nucleotide(const mf_kmerset *ks)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    if (ks->kind != MF_KIND_NUCLEOTIDE) return fail(MF_E_ARG, "record assignment needs a nucleotide bait set");
    return MF_OK;
}

// a record's or group's name into the caller's buffer
static int copy_name(const std::string &nm, char *buf, size_t buflen, size_t *needed)
{
    if (needed) *needed = nm.size() + 1;
    if (!buf || buflen < nm.size() + 1) return fail(MF_E_ARG, "buffer too small: the name needs %llu bytes", (unsigned long long)(nm.size() + 1));
    memcpy(buf, nm.c_str(), nm.size() + 1);
    return MF_OK;
}

extern "C" {

int mf_kmerset_record_count(const mf_kmerset *ks, uint64_t *n_records)
{
    int rc = need_nucleotide(ks); if (rc) return rc;
    if (!n_records) return fail(MF_E_ARG, "n_records is NULL");
    *n_records = ks->bait.rec_len.size();
    return MF_OK;
}

int mf_kmerset_record_name(const mf_kmerset *ks, uint64_t i, char *buf, size_t buflen, size_t *needed)
{
    int rc = need_nucleotide(ks); if (rc) return rc;
    if (i >= ks->bait.names.size()) return fail(MF_E_ARG, "record %llu out of range (the set has %llu)", (unsigned long long)i, (unsigned long long)ks->bait.names.size());
    return copy_name(ks->bait.names[i], buf, buflen, needed);
}

int mf_assign(const mf_kmerset *ks_, const mf_reads *reads_, uint32_t threshold, int mode, uint32_t *out_bits, uint32_t *assign_out,
              uint64_t *record_reads, mf_filter_stats_t *stats)
{
    mf_kmerset *ks = const_cast<mf_kmerset *>(ks_);
    mf_reads *r = const_cast<mf_reads *>(reads_);
    int rc = need_nucleotide(ks); if (rc) return rc;
    if (!r) return fail(MF_E_ARG, "NULL handle");
    rc = filter_common(ks, r, threshold, mode, out_bits, nullptr, 1, stats);
    if (rc) return rc;
    return assign_after_filter(ks, r, assign_out, record_reads, nullptr, false);
}

// ------------------------------------------------------- group assignment
int mf_kmerset_group_records(mf_kmerset *ks, const char *sep, int field)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    if (field < 0) return fail(MF_E_ARG, "field %d is negative", field);
    const bool identity = !sep || field == 0;
    if (!identity && !*sep) return fail(MF_E_ARG, "the separator is empty");
    std::vector<uint32_t> rec_group;
    std::vector<std::string> group_names;
    if (!identity) {          // the field-th sep-separated token of the name (from 1); the whole name when it has fewer fields
        const std::string sp = sep;
        std::map<std::string, uint32_t> index;
        const std::vector<std::string> &names = ks->names();
        rec_group.reserve(names.size());
        for (const std::string &nm : names) {
            size_t at = 0; int f = 1;
            while (f < field) { const size_t q = nm.find(sp, at); if (q == std::string::npos) break; at = q + sp.size(); f++; }
            std::string g = nm;
            if (f == field) { const size_t q = nm.find(sp, at); g = nm.substr(at, q == std::string::npos ? std::string::npos : q - at); }
            auto it = index.find(g);
            if (it == index.end()) { it = index.emplace(g, (uint32_t)group_names.size()).first; group_names.push_back(g); }
            rec_group.push_back(it->second);
        }
    }
    std::lock_guard<std::mutex> lk(ks->mu);
    for (auto &kv : ks->dev)
        if (kv.second.gowner) {
            HIPCHK(hipSetDevice(phys(kv.first)));
            HIPCHK(DevTables::drop(kv.second.gowner));
        }
    ks->rec_group.swap(rec_group);
    ks->group_names.swap(group_names);
    return MF_OK;
}

int mf_kmerset_group_count(const mf_kmerset *ks, uint64_t *n_groups)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    if (!n_groups) return fail(MF_E_ARG, "n_groups is NULL");
    *n_groups = ks->n_groups();
    return MF_OK;
}

int mf_kmerset_group_name(const mf_kmerset *ks, uint64_t i, char *buf, size_t buflen, size_t *needed)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    if (i >= ks->n_groups()) return fail(MF_E_ARG, "group %llu out of range (the set has %llu)", (unsigned long long)i, (unsigned long long)ks->n_groups());
    return copy_name(ks->group_name(i), buf, buflen, needed);
}

int mf_assign_groups(const mf_kmerset *ks_, const mf_reads *reads_, uint32_t threshold, int mode, uint32_t *out_bits, uint32_t *assign_out,
                     uint64_t *group_reads, mf_filter_stats_t *stats)
{
    mf_kmerset *ks = const_cast<mf_kmerset *>(ks_);
    mf_reads *r = const_cast<mf_reads *>(reads_);
    if (!ks || !r) return fail(MF_E_ARG, "NULL handle");
    int rc = filter_common(ks, r, threshold, mode, out_bits, nullptr, 1, stats);
    if (rc) return rc;
    return assign_after_filter(ks, r, assign_out, group_reads, nullptr, true);
}

} // extern "C"

// ------------------------------------------------------------------- k-mer depth
// The depth tables of a set on `device` (nucleotide or protein): made by the first depth call there, under the set's lock.
static int depth_tables(mf_kmerset *ks, int device, DevTables *T)
{
    std::lock_guard<std::mutex> lk(ks->mu);
    if (T->rep) return MF_OK;
    const uint64_t total = ks->positions();
    if (total >= DEPTH_NONE || ks->slots > DEPTH_NONE) return fail(MF_E_ARG, "k-mer depth takes sets of fewer than 2^32 - 1 positions and slots");
    DevCtx *ctx; int rc = get_ctx(device, &ctx); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const bool by_slot = depth_index_option() == 1;
    BaitOnDevice B;
    rc = B.upload(ks, st); if (rc) return rc;
    std::vector<DepthItem> items;
    for (uint32_t j = 0; j < B.n_rec; j++)
        for (uint64_t a = B.starts[j]; a < B.starts[j + 1]; a += DEPTH_ITEM) items.push_back(DepthItem{a, (uint32_t)std::min<uint64_t>(DEPTH_ITEM, B.starts[j + 1] - a), j});
    uint32_t *rep = nullptr, *pos_rep = nullptr; DepthItem *d_items = nullptr;
    HIPCHK(B.tmp.alloc(rep, ks->slots * 4));
    HIPCHK(B.tmp.alloc(pos_rep, std::max<uint64_t>(total, 1) * 4));
    HIPCHK(B.tmp.alloc(d_items, std::max<size_t>(items.size(), 1) * sizeof(DepthItem)));
    if (!items.empty()) HIPCHK(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(DepthItem), hipMemcpyHostToDevice, st));
    HIPCHK(launch_build_depth(B.view, B.aa, T->view, rep, pos_rep, by_slot, st));
    HIPCHK(hipStreamSynchronize(st));
    T->rep = B.tmp.release(rep); T->pos_rep = B.tmp.release(pos_rep); T->ditems = B.tmp.release(d_items);
    T->n_ditems = (uint32_t)items.size(); T->dcnt_n = by_slot ? std::max<uint64_t>(ks->slots, total) : total;
    return MF_OK;
}

// The windows of the reads that passed the filter pass just run on this read set (its bitmap in r->d_bits[r->cur]) added into tot
// (T->dcnt_n u64 counters on r's device, which other read sets there may be adding into at the same time).  Ends synchronised.
static int depth_after_filter(mf_kmerset *ks, mf_reads *r, unsigned long long *tot)
{
    DevTables *T; int rc = build_on_device(ks, r->device, &T); if (rc) return rc;
    rc = depth_tables(ks, r->device, T); if (rc) return rc;
    DevCtx *ctx; rc = get_ctx(r->device, &ctx, r->lane); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n = r->v.n_reads, n_cnt = T->dcnt_n;
    if (!n || !n_cnt) return MF_OK;
    // a 32-bit counter holds every window of the read set unless they could number 2^32: then the windows go straight into tot
    const uint64_t span = ks->kind == MF_KIND_PROTEIN ? 3 * (uint64_t)ks->k : (uint64_t)ks->k;
    const uint64_t per = r->v.uniform_len ? (r->v.uniform_len >= span ? r->v.uniform_len - span + 1 : 0) : 0;
    const uint64_t bound = (r->v.uniform_len ? n * per : r->v.total_bases) * (ks->kind == MF_KIND_PROTEIN ? 2 : 1);
    const bool wide = bound >= DEPTH_NONE;
    HIPCHK(dev_reserve(r->d_acnt, r->cap_acnt, 8, false));
    HIPCHK(hipMemsetAsync(r->d_acnt, 0, 8, st));
    HIPCHK(dev_reserve(r->d_alist, r->cap_alist, n * 4, true));
    if (!wide) { HIPCHK(dev_reserve(r->d_rpos, r->cap_rpos, n_cnt * 4, false)); HIPCHK(hipMemsetAsync(r->d_rpos, 0, n_cnt * 4, st)); }
    HIPCHK(launch_pass_list(r->d_bits[r->cur], n, r->d_alist, r->d_acnt, st));
    HIPCHK(launch_depth_count(r->v, T->view, T->rep, r->d_alist, r->d_acnt, wide ? nullptr : r->rpos_u32(), wide ? tot : nullptr, ctx->n_cu, st));
    if (!wide) HIPCHK(launch_depth_fold(r->rpos_u32(), n_cnt, tot, st));
    HIPCHK(hipStreamSynchronize(st));
    return MF_OK;
}

// What a report's last step works in on the device.  A resident call fills it from the read set's cached buffers (dev_reserve: a warm
// call allocates nothing), a file-level call from temporaries of its own (DevScratch).
struct DepthScratch {
    uint32_t *prof; unsigned long long *rec;          // the profile, the record sums
    static size_t prof_bytes(const mf_kmerset *ks) { return std::max<uint64_t>(ks->positions(), 1) * 4; }
    static size_t rec_bytes(const mf_kmerset *ks) { return std::max<size_t>(ks->rec_len().size(), 1) * 32; }
};

// The profile (ks->positions() u32) and the record summaries (R entries) from the totals tot on `device` (stream st); each optional.
static int depth_report(mf_kmerset *ks, int device, hipStream_t st, const unsigned long long *tot, DepthScratch s, uint32_t *profile, mf_depth_record_t *records)
{
    DevTables *T; int rc = build_on_device(ks, device, &T); if (rc) return rc;
    rc = depth_tables(ks, device, T); if (rc) return rc;
    const uint64_t total = ks->positions(), n_rec = ks->rec_len().size();
    if (records && n_rec) HIPCHK(hipMemsetAsync(s.rec, 0, n_rec * 32, st));
    if (profile && total) HIPCHK(hipMemsetAsync(s.prof, 0xFF, total * 4, st));          // (records with no item: none, they are empty)
    HIPCHK(launch_depth_profile(T->ditems, T->n_ditems, T->pos_rep, tot, profile ? s.prof : nullptr, records ? s.rec : nullptr, st));
    if (profile && total) HIPCHK(hipMemcpyAsync(profile, s.prof, total * 4, hipMemcpyDeviceToHost, st));
    if (records && n_rec) HIPCHK(hipMemcpyAsync(records, s.rec, n_rec * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MF_OK;
}

extern "C" {

int mf_kmerset_record_starts(const mf_kmerset *ks, uint64_t *starts, size_t n, size_t *needed)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    const std::vector<uint64_t> s = record_starts(ks);
    if (needed) *needed = s.size();
    if (!starts || n < s.size()) return fail(MF_E_ARG, "buffer too small: the set has %llu records, %llu offsets", (unsigned long long)(s.size() - 1), (unsigned long long)s.size());
    std::copy(s.begin(), s.end(), starts);
    return MF_OK;
}

int mf_depth(const mf_kmerset *ks_, const mf_reads *reads_, uint32_t threshold, int mode, uint32_t *out_bits, uint32_t *profile,
             mf_depth_record_t *records, mf_filter_stats_t *stats)
{
    mf_kmerset *ks = const_cast<mf_kmerset *>(ks_);
    mf_reads *r = const_cast<mf_reads *>(reads_);
    if (!ks || !r) return fail(MF_E_ARG, "NULL handle");
    int rc = filter_common(ks, r, threshold, mode, out_bits, nullptr, 1, stats);
    if (rc) return rc;
    DevTables *T; rc = build_on_device(ks, r->device, &T); if (rc) return rc;
    rc = depth_tables(ks, r->device, T); if (rc) return rc;
    DevCtx *ctx; rc = get_ctx(r->device, &ctx, r->lane); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n_cnt = T->dcnt_n;
    HIPCHK(dev_reserve(r->d_rtot, r->cap_rtot, std::max<uint64_t>(n_cnt, 1) * 8, false));
    HIPCHK(hipMemsetAsync(r->d_rtot, 0, std::max<uint64_t>(n_cnt, 1) * 8, st));
    rc = depth_after_filter(ks, r, r->d_rtot); if (rc) return rc;
    // (the profile goes through the pass's 32-bit counters, which the totals have taken up: never a smaller buffer than theirs)
    HIPCHK(dev_reserve(r->d_rpos, r->cap_rpos, std::max<size_t>(n_cnt * 4, DepthScratch::prof_bytes(ks)), false));
    HIPCHK(dev_reserve(r->d_rsum, r->cap_rsum, DepthScratch::rec_bytes(ks), false));
    return depth_report(ks, r->device, st, r->d_rtot, DepthScratch{r->rpos_u32(), r->d_rsum}, profile, records);
}

} // extern "C"

// ------------------------------------------------------------------- placement
// The anchor table of a nucleotide set on `device`, and the record starts beside it: made by the first placement call there, under the
// set's lock.
static int place_tables(mf_kmerset *ks, int device, DevTables *T)
{
    std::lock_guard<std::mutex> lk(ks->mu);
    if (T->place_built) return MF_OK;
    if (ks->positions() >= 0x7FFFFFFFull || ks->rec_len().size() >= (1ull << 30))
        return fail(MF_E_ARG, "placement takes sets of fewer than 2^31 - 1 positions and 2^30 records");
    DevCtx *ctx; int rc = get_ctx(device, &ctx); if (rc) return rc;
    hipStream_t st = ctx->stream;
    BaitOnDevice B;
    rc = B.upload(ks, st); if (rc) return rc;
    uint32_t *lo = nullptr, *hi = nullptr; Anchor *anchor = nullptr;
    HIPCHK(B.tmp.alloc(lo, ks->slots * 4));
    HIPCHK(B.tmp.alloc(hi, ks->slots * 4));
    HIPCHK(B.tmp.alloc(anchor, ks->slots * 8));
    HIPCHK(launch_build_anchor(B.view, B.rec_start, B.n_rec, T->view, anchor, lo, hi, st));
    HIPCHK(hipStreamSynchronize(st));
    T->anchor = B.tmp.release(anchor); T->place_starts = B.tmp.release(const_cast<uint64_t *>(B.rec_start));
    T->place_built = true;
    return MF_OK;
}

// The bait's packed bases and run lengths beside the anchor table, and its validity one bit a position (runlen != 0): kept by the first
// pile-up or verifying call on `device`, under the set's lock.  The packed bases and the validity bits are each padded by a zero word:
// the second word of the 16-base compare's funnel read (mf_score.h) exists wherever its first does.
static int pileup_tables(mf_kmerset *ks, int device, DevTables *T)
{
    int rc = place_tables(ks, device, T); if (rc) return rc;
    std::lock_guard<std::mutex> lk(ks->mu);
    if (T->pile_built) return MF_OK;
    DevCtx *ctx; rc = get_ctx(device, &ctx); if (rc) return rc;
    hipStream_t st = ctx->stream;
    DevScratch tmp;
    uint32_t *words = nullptr, *valid = nullptr; uint8_t *runlen = nullptr;
    const size_t total = (size_t)ks->bait.total, n_words = std::max(ks->bait.words.size(), (total + 15) / 16) + 1, n_valid = (total + 31) / 32 + 1;
    std::vector<uint32_t> h_valid(n_valid, 0);
    for (size_t p = 0; p < total; p++) if (ks->bait.runlen[p]) h_valid[p >> 5] |= 1u << (p & 31);
    HIPCHK(tmp.alloc(words, n_words * 4));
    HIPCHK(tmp.alloc(valid, n_valid * 4));
    HIPCHK(tmp.alloc(runlen, std::max<size_t>(ks->bait.runlen.size(), 1)));
    HIPCHK(hipMemsetAsync(words, 0, n_words * 4, st));
    if (!ks->bait.words.empty()) HIPCHK(hipMemcpyAsync(words, ks->bait.words.data(), ks->bait.words.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(valid, h_valid.data(), n_valid * 4, hipMemcpyHostToDevice, st));
    if (!ks->bait.runlen.empty()) HIPCHK(hipMemcpyAsync(runlen, ks->bait.runlen.data(), ks->bait.runlen.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    T->pile_words = tmp.release(words); T->pile_runlen = tmp.release(runlen); T->pile_valid = tmp.release(valid);
    T->pile_words_n = n_words; T->pile_valid_n = n_valid;
    T->pile_built = true;
    return MF_OK;
}

static int pile_nomem(size_t words) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the pile-up counters need %llu bytes on the device", (unsigned long long)(words * 8)); }
static int gap_nomem(size_t words) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the pile-up counters and the insertion pile need %llu bytes on the device", (unsigned long long)(words * 8)); }
static int ext_nomem(size_t words) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the pile-up counters, the insertion pile and the extension pile need %llu bytes on the device", (unsigned long long)(words * 8)); }

// Everything a call of the placement family is asked for: mf_place, mf_pileup, mf_verify and their file-level calls are each one of
// these and one call of a driver below.  family: the name the messages use.  with_pileup: the layout holds pile-up counters.  A family
// that takes no cut leaves min_depth and max_permille as they are here.  Every output is optional; a file-level call has no per-read ones.
// keep (verifying families): the keep mode, MF_KEEP_*; keep_bits (resident): the pass bits amended by it, n_reads bits.
struct PlaceRequest {
    const char *family; bool verify, with_pileup;
    uint32_t min_depth = 1, max_permille = 1000;
    mf_place_t *place_out = nullptr; mf_score_t *score_out = nullptr;
    uint32_t *base_depth = nullptr; mf_place_record_t *place_records = nullptr;
    mf_pileup_t *pileup = nullptr; uint8_t *consensus = nullptr; mf_pileup_record_t *pileup_records = nullptr;
    mf_score_record_t *score_records = nullptr; uint64_t *unplaced = nullptr;
    int keep = MF_KEEP_PASSING; uint32_t *keep_bits = nullptr;
    // an aligning family (a verifying one): the band, and what it gives in place of the scores
    bool align = false; uint32_t band = 0;
    mf_align_t *align_out = nullptr; mf_indel_t *indels = nullptr; mf_align_record_t *align_records = nullptr;
    // a gapped aligning family: the insertion pile (positions * 2 * band entries), the gapped consensus (room for positions * (1 + 2 * band)
    // bytes), its R + 1 record offsets and its record summaries.  All null: the aligning family as it was.
    mf_pileup_t *ins_pile = nullptr; uint8_t *gapped = nullptr; uint64_t *gapped_starts = nullptr; mf_gapped_record_t *gapped_records = nullptr;
    // an extending family (a gapped one): the columns an end, the extension pile (R * 2 * extend entries), the extended records (room for
    // positions * (1 + 2 * band) + 2 * R * extend bytes), their R + 1 offsets and their summaries.  extend 0: the gapped family as it was.
    uint32_t extend = 0;
    mf_pileup_t *ext_pile = nullptr; uint8_t *extended = nullptr; uint64_t *extended_starts = nullptr; mf_extend_record_t *extend_records = nullptr;
    bool ext_asked() const { return ext_pile || extended || extended_starts || extend_records; }
    bool ext() const { return align && extend && ext_asked(); }
    bool gap() const { return align && (ins_pile || gapped || gapped_starts || gapped_records || ext()); }
    int (*nomem() const)(size_t) { return ext() ? ext_nomem : gap() ? gap_nomem : with_pileup ? pile_nomem : nullptr; }
    // the one argument check of the family (a resident call checks its read set behind it)
    int check(const mf_kmerset *ks) const
    {
        if (max_permille > 1000) return fail(MF_E_ARG, "max_permille is %u: the cut is a number from 0 to 1000", max_permille);
        if (min_depth == 0) return fail(MF_E_ARG, "min_depth is 0: a called position needs at least one base");
        if (keep < MF_KEEP_PASSING || keep > MF_KEEP_PLACED) return fail(MF_E_ARG, "keep is %d: the keep mode is MF_KEEP_PASSING (0), MF_KEEP_ACCEPTED (1) or MF_KEEP_PLACED (2)", keep);
        if (align && band > ALIGN_MAX_BAND) return fail(MF_E_ARG, "band is %u: the band is a number from 0 to %u and below k", band, ALIGN_MAX_BAND);
        if (extend > MF_EXTEND_MAX) return fail(MF_E_ARG, "extend is %u: a record grows by 0 to %u columns an end", extend, (unsigned)MF_EXTEND_MAX);
        if (!extend && ext_asked()) return fail(MF_E_ARG, "extend is 0: ext_pile, extended, extended_starts and extend_records must be NULL");
        if (!ks) return fail(MF_E_ARG, "NULL handle");
        if (ks->kind != MF_KIND_NUCLEOTIDE) return fail(MF_E_ARG, "%s needs a nucleotide bait set", family);
        if (align && !align_band_ok(band, ks->k)) return fail(MF_E_ARG, "band is %u: the band stays below k = %d", band, ks->k);
        return MF_OK;
    }
    PlaceLayout layout(const mf_kmerset *ks) const { return PlaceLayout(ks->positions(), ks->rec_len().size(), with_pileup, verify, max_permille, align, band, gap(), ext() ? extend : 0); }
    ReportScratch scratch(const mf_kmerset *ks) const
    {
        return ReportScratch(ks->positions(), ks->rec_len().size(), place_scan_tiles(ks->positions()), base_depth || place_records || gap(), with_pileup,
                             gap() ? (int)(2 * band) : -1, ext() ? extend : 0);
    }
};

// the tables on `device` that the kernels of a placement of layout L read
static int placement_tables(mf_kmerset *ks, int device, const PlaceLayout &L, DevTables **T)
{
    int rc = build_on_device(ks, device, T); if (rc) return rc;
    return L.verify || L.n_pile ? pileup_tables(ks, device, *T) : place_tables(ks, device, *T);
}

// The reads that passed the filter pass just run on this read set (its bitmap in r->d_bits[r->cur]) placed: their footprints, their
// records' counters and (with a pile-up) their bases into the counters t of layout L (on r's device; other read sets there may be adding
// into them at the same time), their placements into place (optional, initialised, n_reads entries on the device); *listed: how many
// passed.  A verifying layout: every placed read is scored first and cut at L.max_permille; score (optional, zeroed, n_reads entries on
// the device) takes the scores.  keep_dev (optional, a verifying layout only): the read set's keep bitmap, a copy of the pass bitmap,
// in which the kernel clears the bits of the reads the keep mode `keep` does not write (keep_clears, mf_score.h).  An aligning layout:
// the placed reads are aligned inside L.band instead (launch_align, in the read set's work memory d_awork); align (optional, zeroed,
// n_reads entries on the device) takes the alignments and score stays null; *longest (optional): the set's longest read, which sized the
// work memory.  Ends synchronised.
static int place_after_filter(mf_kmerset *ks, mf_reads *r, const PlaceLayout &L, unsigned long long *t, PlaceOut *place, ScoreOut *score, uint64_t *listed,
                              uint32_t *keep_dev = nullptr, int keep = MF_KEEP_PASSING, AlignOut *align = nullptr, uint64_t *longest = nullptr)
{
    DevTables *T; int rc = placement_tables(ks, r->device, L, &T); if (rc) return rc;
    DevCtx *ctx; rc = get_ctx(r->device, &ctx, r->lane); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n = r->v.n_reads;
    *listed = 0;
    if (!n) return MF_OK;
    HIPCHK(dev_reserve(r->d_acnt, r->cap_acnt, 8, false));
    // start and end are 32-bit: a read must end below 2^31 wherever it lies on the bait
    const uint64_t room = 0x80000000ull - ks->positions();
    unsigned long long v = 0;
    bool too_long = r->v.uniform_len >= room;
    if (!r->v.uniform_len && (r->v.total_bases >= room || L.align)) {          // only then can a ragged set hold such a read; the alignment's work memory goes by the longest
        HIPCHK(hipMemsetAsync(r->d_acnt, 0, 8, st));
        HIPCHK(launch_max_read_len(r->v.offsets, n, r->d_acnt, st));
        HIPCHK(hipMemcpyAsync(&v, r->d_acnt, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        too_long = v >= room;
    }
    if (too_long) return fail(MF_E_ARG, "placement takes reads of fewer than 2^31 - positions bases (%llu for this set)", (unsigned long long)room);
    HIPCHK(hipMemsetAsync(r->d_acnt, 0, 8, st));
    HIPCHK(dev_reserve(r->d_alist, r->cap_alist, n * 4, true));
    HIPCHK(launch_pass_list(r->d_bits[r->cur], n, r->d_alist, r->d_acnt, st));
    PlaceCut cut{};
    if (L.verify || L.align) cut = PlaceCut{ScoreBait{T->pile_words, T->pile_words_n - 1, T->pile_valid, T->pile_valid_n - 1}, L.max_permille, L.score_sums(t), keep_dev, keep};
    if (L.align) {
        const uint64_t max_len = r->v.uniform_len ? r->v.uniform_len : v;
        if (longest) *longest = max_len;
        const size_t bytes = (size_t)(align_waves(n, max_len, ctx->n_cu) * align_work_words(max_len)) * 8;
        const hipError_t e = dev_reserve(r->d_awork, r->cap_awork, bytes, false);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the alignment of reads of up to %llu bases needs %llu bytes on the device", (unsigned long long)max_len, (unsigned long long)bytes); }
        HIPCHK(e);
        const PlaceAlign pa{cut, L.band, align, L.indel(t), r->d_awork, max_len, L.ins(t), L.ext(t), L.extend};
        HIPCHK(launch_align(r->v, T->view, T->anchor, T->place_starts, r->d_alist, r->d_acnt, (uint32_t)ks->rec_len().size(), place, L.diff(t), L.cnt(t), L.pile(t),
                            pa, ctx->n_cu, st));
    } else {
        const PlaceVerify pv{cut, score};
        HIPCHK(launch_place(r->v, T->view, T->anchor, T->place_starts, r->d_alist, r->d_acnt, (uint32_t)ks->rec_len().size(), place, L.diff(t), L.cnt(t), L.pile(t),
                            L.verify ? &pv : nullptr, ctx->n_cu, st));
    }
    HIPCHK(hipMemcpyAsync(&v, r->d_acnt, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *listed = v;
    return MF_OK;
}

// The keep bitmap of the pass just run on this read set, for a keep mode other than MF_KEEP_PASSING: r->d_keep (reserved once: a warm
// call allocates nothing) as a device-to-device copy of the pass bitmap, enqueued on st.  *keep_dev stays null for MF_KEEP_PASSING and
// for an empty read set: no bitmap is handed to the kernel.
static int keep_bitmap(mf_reads *r, int keep, hipStream_t st, uint32_t **keep_dev)
{
    *keep_dev = nullptr;
    const uint64_t n = r->v.n_reads;
    if (keep == MF_KEEP_PASSING || !n) return MF_OK;
    HIPCHK(dev_reserve(r->d_keep, r->cap_keep, r->bitmap_bytes, true));
    HIPCHK(hipMemcpyAsync(r->d_keep, r->d_bits[r->cur], (size_t)((n + 31) / 32) * 4, hipMemcpyDeviceToDevice, st));
    *keep_dev = r->d_keep;
    return MF_OK;
}

// Every report the request q asks for from the counters t of layout L on `device` (stream st), worked out in the sections S of the two
// scratch buffers sums and pos: base depth (positions u32) and placement's record summaries, the called pile-up (positions entries), the
// consensus (positions bytes) and the pile-up's record summaries, the records' scores, and unplaced[2] -- the passing reads that are not
// placed, then not_passing as it is given.  Both kernels and every copy are enqueued, then the stream is waited for once.
static int placement_report(mf_kmerset *ks, int device, hipStream_t st, const PlaceLayout &L, unsigned long long *t, const PlaceRequest &q,
                            const ReportScratch &S, unsigned long long *sums, void *pos, uint64_t not_passing)
{
    static_assert(sizeof(mf_place_t) == 24 && sizeof(PlaceOut) == 24 && sizeof(mf_place_record_t) == 48, "placement records");
    static_assert(sizeof(mf_pileup_t) == 16 && sizeof(PileOut) == 16 && sizeof(mf_pileup_record_t) == 8 * PILE_SUMS, "pile-up records");
    static_assert(sizeof(mf_score_t) == 8 && sizeof(ScoreOut) == 8 && sizeof(mf_score_record_t) == 8 * (4 + MF_SCORE_BINS) && MF_SCORE_BINS == SCORE_BINS, "score records");
    static_assert(sizeof(mf_align_t) == 24 && sizeof(AlignOut) == 24 && sizeof(mf_indel_t) == 12 && sizeof(mf_align_record_t) == 8 * (7 + MF_SCORE_BINS), "align records");
    static_assert(sizeof(mf_gapped_record_t) == 8 * GAPPED_SUMS && sizeof(mf_extend_record_t) == 40, "gapped and extend records");
    static_assert(ALIGN_SUMS == ALIGN_RECORD_SUMS && ALIGN_INDEL == ALIGN_POSITION_COUNTERS, "the kernel's counters are the layout's");
    DevTables *T; int rc = placement_tables(ks, device, L, &T); if (rc) return rc;
    const uint64_t total = ks->positions(), n_rec = L.n_rec;
    std::vector<unsigned long long> h_cnt(L.n_cnt + (q.score_records || q.align_records ? L.n_score() : 0), 0), h_sum(2 * n_rec + 1, 0), h_indel(q.indels ? L.n_indel : 0, 0);
    if (q.base_depth || q.place_records) {
        unsigned long long *work = S.work.in<unsigned long long>(sums); uint32_t *depth = S.depth.in<uint32_t>(pos);
        if (q.place_records && n_rec) HIPCHK(hipMemsetAsync(work, 0, 2 * n_rec * 8, st));
        HIPCHK(launch_place_profile(L.diff(t), total, T->place_starts, (uint32_t)n_rec, work + 2 * n_rec, q.base_depth ? depth : nullptr,
                                    q.place_records ? work : nullptr, st));
        if (q.base_depth && total) HIPCHK(hipMemcpyAsync(q.base_depth, depth, total * 4, hipMemcpyDeviceToHost, st));
        if (q.place_records && n_rec) HIPCHK(hipMemcpyAsync(h_sum.data(), work, 2 * n_rec * 8, hipMemcpyDeviceToHost, st));
    }
    const bool gap = q.gap();          // (the gapped call reads the consensus bytes on the device, asked for or not)
    const bool ext = q.ext();          // (the extended records hold the gapped bytes, asked for or not)
    std::vector<uint8_t> h_gcount, h_gbytes, h_ebytes; std::vector<unsigned long long> h_gsum, h_esum;
    if (q.with_pileup && (q.pileup || q.consensus || q.pileup_records || gap)) {
        unsigned long long *psums = S.pile_sums.in<unsigned long long>(sums); PileOut *out = S.pile_out.in<PileOut>(pos); uint8_t *cons = S.consensus.in<uint8_t>(pos);
        if (q.pileup_records && n_rec) HIPCHK(hipMemsetAsync(psums, 0, PILE_SUMS * n_rec * 8, st));
        HIPCHK(launch_pileup_call(L.pile(t), BaitView{T->pile_words, total, T->pile_runlen}, T->place_starts, (uint32_t)n_rec, q.min_depth,
                                  q.pileup ? out : nullptr, q.consensus || gap ? cons : nullptr, q.pileup_records ? psums : nullptr, st));
        if (q.pileup && total) HIPCHK(hipMemcpyAsync(q.pileup, out, total * sizeof(PileOut), hipMemcpyDeviceToHost, st));
        if (q.consensus && total) HIPCHK(hipMemcpyAsync(q.consensus, cons, total, hipMemcpyDeviceToHost, st));
        if (q.pileup_records && n_rec) HIPCHK(hipMemcpyAsync(q.pileup_records, psums, PILE_SUMS * n_rec * 8, hipMemcpyDeviceToHost, st));
    }
    const size_t span = L.span();
    const bool call = gap && (q.gapped || q.gapped_starts || q.extended || q.extended_starts || q.extend_records);          // (the gapped record summaries come from the kernel's sums)
    if (gap) {
        unsigned long long *work = S.work.in<unsigned long long>(sums), *gsums = S.gap_sums.in<unsigned long long>(sums);
        PileOut *ins_out = S.ins_out.in<PileOut>(pos); uint8_t *gcount = S.gap_count.in<uint8_t>(pos), *gbytes = S.gap_bytes.in<uint8_t>(pos);
        if (n_rec) HIPCHK(hipMemsetAsync(gsums, 0, GAPPED_SUMS * n_rec * 8, st));
        HIPCHK(launch_gapped_call(L.diff(t), total, L.indel(t), L.ins(t), (uint32_t)span, S.consensus.in<uint8_t>(pos), T->place_starts, (uint32_t)n_rec, q.min_depth,
                                  work + 2 * n_rec, q.ins_pile ? ins_out : nullptr, gcount, gbytes, gsums, st));
        if (q.ins_pile && total && span) HIPCHK(hipMemcpyAsync(q.ins_pile, ins_out, total * span * sizeof(PileOut), hipMemcpyDeviceToHost, st));
        if (call && total) {
            h_gcount.resize(total); h_gbytes.resize(total * (1 + span));
            HIPCHK(hipMemcpyAsync(h_gcount.data(), gcount, total, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_gbytes.data(), gbytes, h_gbytes.size(), hipMemcpyDeviceToHost, st));
        }
        if (q.gapped_records && n_rec) { h_gsum.resize(GAPPED_SUMS * n_rec); HIPCHK(hipMemcpyAsync(h_gsum.data(), gsums, h_gsum.size() * 8, hipMemcpyDeviceToHost, st)); }
    }
    const size_t E = L.extend, n_ends = 2 * n_rec;
    if (ext && n_rec) {          // both ends of every record called, once, from the sums
        unsigned long long *esums = S.ext_sums.in<unsigned long long>(sums);
        PileOut *ext_out = S.ext_out.in<PileOut>(pos); uint8_t *ebytes = S.ext_bytes.in<uint8_t>(pos);
        HIPCHK(launch_extend_call(L.ext(t), (uint32_t)E, (uint32_t)n_rec, q.min_depth, q.ext_pile ? ext_out : nullptr, ebytes, esums, st));
        if (q.ext_pile) HIPCHK(hipMemcpyAsync(q.ext_pile, ext_out, n_ends * E * sizeof(PileOut), hipMemcpyDeviceToHost, st));
        h_ebytes.resize(n_ends * E); h_esum.resize(EXTEND_END_SUMS * n_ends);
        HIPCHK(hipMemcpyAsync(h_ebytes.data(), ebytes, h_ebytes.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_esum.data(), esums, h_esum.size() * 8, hipMemcpyDeviceToHost, st));
    }
    if (!h_indel.empty()) HIPCHK(hipMemcpyAsync(h_indel.data(), L.indel(t), h_indel.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_cnt.data(), L.cnt(t), h_cnt.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t p = 0; p < h_indel.size() / ALIGN_INDEL; p++)          // (clamped like the depth)
        q.indels[p] = mf_indel_t{clamp_count(h_indel[ALIGN_INDEL * p]), clamp_count(h_indel[ALIGN_INDEL * p + 1]), clamp_count(h_indel[ALIGN_INDEL * p + 2])};
    if (call) {          // the positions' bytes, concatenated record by record; an extending call: between the bytes its ends emit
        const std::vector<uint64_t> starts = record_starts(ks);
        uint64_t at = 0, xat = 0;
        for (uint64_t j = 0; j < n_rec; j++) {
            if (q.gapped_starts) q.gapped_starts[j] = at;
            const uint64_t at0 = at;
            // (the begin columns from the farthest to the one next to the record)
            const size_t nb = ext ? std::min<size_t>(h_esum[EXTEND_END_SUMS * (2 * j)], E) : 0, ne = ext ? std::min<size_t>(h_esum[EXTEND_END_SUMS * (2 * j + 1)], E) : 0;
            if (ext && q.extended_starts) q.extended_starts[j] = xat;
            if (ext && q.extended) for (size_t e = 0; e < nb; e++) q.extended[xat + e] = h_ebytes[(2 * j) * E + (nb - 1 - e)];
            xat += nb;
            for (uint64_t p = starts[j]; p < starts[j + 1]; p++) {
                const size_t m = std::min<size_t>(h_gcount[p], 1 + span);
                if (q.gapped) memcpy(q.gapped + at, h_gbytes.data() + p * (1 + span), m);
                if (ext && q.extended) memcpy(q.extended + xat, h_gbytes.data() + p * (1 + span), m);
                at += m; xat += m;
            }
            if (ext && q.extended) memcpy(q.extended + xat, h_ebytes.data() + (2 * j + 1) * E, ne);
            xat += ne;
            if (ext && q.extend_records)
                q.extend_records[j] = mf_extend_record_t{at - at0 + nb + ne, nb, ne, h_esum[EXTEND_END_SUMS * (2 * j) + 1], h_esum[EXTEND_END_SUMS * (2 * j + 1) + 1]};
        }
        if (q.gapped_starts) q.gapped_starts[n_rec] = at;
        if (ext && q.extended_starts) q.extended_starts[n_rec] = xat;
    }
    for (size_t j = 0; j < h_gsum.size() / GAPPED_SUMS; j++)
        q.gapped_records[j] = mf_gapped_record_t{h_gsum[GAPPED_SUMS * j], h_gsum[GAPPED_SUMS * j + 1], h_gsum[GAPPED_SUMS * j + 2], h_gsum[GAPPED_SUMS * j + 3]};
    if (q.align_records) L.align_records(h_cnt.data(), q.align_records);
    if (q.place_records)
        for (uint64_t j = 0; j < n_rec; j++)
            q.place_records[j] = mf_place_record_t{h_cnt[4 * j], h_cnt[4 * j + 1], h_cnt[4 * j + 2], h_cnt[4 * j + 3], h_sum[2 * j], h_sum[2 * j + 1]};
    if (q.score_records) L.score_records(h_cnt.data(), q.score_records);
    if (q.unplaced) { q.unplaced[0] = h_cnt[4 * n_rec]; q.unplaced[1] = not_passing; }
    return MF_OK;
}

// The resident call of the family: one filter pass, the passing reads placed into the read set's cached buffers, the report.
static int placement_resident(const mf_kmerset *ks_, const mf_reads *reads_, uint32_t threshold, int mode, uint32_t *out_bits, mf_filter_stats_t *stats,
                              const PlaceRequest &q)
{
    mf_kmerset *ks = const_cast<mf_kmerset *>(ks_);
    mf_reads *r = const_cast<mf_reads *>(reads_);
    int rc = q.check(ks); if (rc) return rc;
    if (!r) return fail(MF_E_ARG, "NULL handle");
    rc = filter_common(ks, r, threshold, mode, out_bits, nullptr, 1, stats);
    if (rc) return rc;
    DevCtx *ctx; rc = get_ctx(r->device, &ctx, r->lane); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n = r->v.n_reads;
    const PlaceLayout L = q.layout(ks);
    const ReportScratch S = q.scratch(ks);
    const hipError_t e = dev_reserve(r->d_rtot, r->cap_rtot, L.words() * 8, false);
    if (e == hipErrorOutOfMemory && q.nomem()) return q.nomem()(L.words());
    HIPCHK(e);
    HIPCHK(dev_reserve(r->d_rsum, r->cap_rsum, S.sums_bytes, false));
    const hipError_t e2 = dev_reserve(r->d_rpos, r->cap_rpos, S.pos_bytes, false);
    if (e2 == hipErrorOutOfMemory && q.gap()) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the gapped consensus needs %llu bytes on the device", (unsigned long long)S.pos_bytes); }
    HIPCHK(e2);
    HIPCHK(hipMemsetAsync(r->d_rtot, 0, L.words() * 8, st));
    PlaceOut *d_place = nullptr; ScoreOut *d_score = nullptr;
    if (q.place_out && n) {
        HIPCHK(dev_reserve(r->d_place, r->cap_place, n * sizeof(PlaceOut), true));
        HIPCHK(launch_place_init(d_place = r->d_place, n, st));
    }
    if (q.score_out && n) {
        HIPCHK(dev_reserve(r->d_score, r->cap_score, n * sizeof(ScoreOut), true));
        HIPCHK(hipMemsetAsync(d_score = r->d_score, 0, n * sizeof(ScoreOut), st));
    }
    AlignOut *d_align = nullptr;
    if (q.align_out && n) {
        HIPCHK(dev_reserve(r->d_align, r->cap_align, n * sizeof(AlignOut), true));
        HIPCHK(hipMemsetAsync(d_align = r->d_align, 0, n * sizeof(AlignOut), st));
    }
    uint64_t listed = 0;
    uint32_t *d_keep = nullptr;
    rc = keep_bitmap(r, q.keep, st, &d_keep); if (rc) return rc;
    rc = place_after_filter(ks, r, L, r->d_rtot, d_place, d_score, &listed, d_keep, q.keep, d_align); if (rc) return rc;
    // (MF_KEEP_PASSING: keep_bits are the pass bits)
    if (q.keep_bits && n) HIPCHK(hipMemcpyAsync(q.keep_bits, d_keep ? d_keep : r->d_bits[r->cur], (size_t)((n + 31) / 32) * 4, hipMemcpyDeviceToHost, st));
    if (d_place) HIPCHK(hipMemcpyAsync(q.place_out, d_place, n * sizeof(PlaceOut), hipMemcpyDeviceToHost, st));
    if (d_score) HIPCHK(hipMemcpyAsync(q.score_out, d_score, n * sizeof(ScoreOut), hipMemcpyDeviceToHost, st));
    if (d_align) HIPCHK(hipMemcpyAsync(q.align_out, d_align, n * sizeof(AlignOut), hipMemcpyDeviceToHost, st));
    return placement_report(ks, r->device, st, L, r->d_rtot, q, S, r->d_rsum, r->d_rpos, n - listed);
}

extern "C" {

int mf_kmerset_bait_letters(const mf_kmerset *ks, uint8_t *letters, size_t n, size_t *needed)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    if (ks->kind != MF_KIND_NUCLEOTIDE) return fail(MF_E_ARG, "bait letters need a nucleotide bait set");
    const size_t total = (size_t)ks->bait.total;
    if (needed) *needed = total;
    if ((!letters && total) || n < total) return fail(MF_E_ARG, "buffer too small: the set has %llu positions", (unsigned long long)total);
    for (size_t p = 0; p < total; p++)
        letters[p] = ks->bait.runlen[p] ? (uint8_t)"ACGT"[(ks->bait.words[p >> 4] >> (2 * (p & 15))) & 3u] : (uint8_t)'N';
    return MF_OK;
}

int mf_place(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t *out_bits, mf_place_t *place_out,
             uint32_t *base_depth, mf_place_record_t *records, uint64_t *unplaced, mf_filter_stats_t *stats)
{
    PlaceRequest q{"placement", false, false};
    q.place_out = place_out; q.base_depth = base_depth; q.place_records = records; q.unplaced = unplaced;
    return placement_resident(ks, reads, threshold, mode, out_bits, stats, q);
}

int mf_pileup(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t *out_bits,
              mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *records, uint64_t *unplaced, mf_filter_stats_t *stats)
{
    PlaceRequest q{"the pile-up", false, true};
    q.min_depth = min_depth; q.pileup = pileup; q.consensus = consensus; q.pileup_records = records; q.unplaced = unplaced;
    return placement_resident(ks, reads, threshold, mode, out_bits, stats, q);
}

int mf_verify_keep(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille, int keep,
                   uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_score_t *score_out, uint32_t *base_depth,
                   mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records,
                   mf_score_record_t *score_records, uint64_t *unplaced, mf_filter_stats_t *stats)
{
    PlaceRequest q{"verification", true, pileup || consensus || pileup_records};
    q.min_depth = min_depth; q.max_permille = max_permille; q.keep = keep; q.keep_bits = keep_bits;
    q.place_out = place_out; q.score_out = score_out; q.base_depth = base_depth; q.place_records = place_records;
    q.pileup = pileup; q.consensus = consensus; q.pileup_records = pileup_records; q.score_records = score_records; q.unplaced = unplaced;
    return placement_resident(ks, reads, threshold, mode, out_bits, stats, q);
}

int mf_align(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille, int keep, uint32_t band,
             uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_align_t *align_out, uint32_t *base_depth, mf_place_record_t *place_records,
             mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records,
             uint64_t *unplaced, mf_filter_stats_t *stats)
{
    return mf_align_gapped(ks, reads, threshold, mode, min_depth, max_permille, keep, band, out_bits, keep_bits, place_out, align_out, base_depth, place_records,
                           pileup, consensus, pileup_records, indels, align_records, nullptr, nullptr, nullptr, nullptr, unplaced, stats);
}

int mf_align_gapped(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille, int keep, uint32_t band,
                    uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_align_t *align_out, uint32_t *base_depth, mf_place_record_t *place_records,
                    mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records,
                    mf_pileup_t *ins_pile, uint8_t *gapped, uint64_t *gapped_starts, mf_gapped_record_t *gapped_records, uint64_t *unplaced, mf_filter_stats_t *stats)
{
    return mf_align_extended(ks, reads, threshold, mode, min_depth, max_permille, keep, band, 0, out_bits, keep_bits, place_out, align_out, base_depth, place_records,
                             pileup, consensus, pileup_records, indels, align_records, ins_pile, gapped, gapped_starts, gapped_records, nullptr, nullptr, nullptr, nullptr,
                             unplaced, stats);
}

int mf_align_extended(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille, int keep, uint32_t band,
                      uint32_t extend, uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_align_t *align_out, uint32_t *base_depth,
                      mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_indel_t *indels,
                      mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped, uint64_t *gapped_starts, mf_gapped_record_t *gapped_records,
                      mf_pileup_t *ext_pile, uint8_t *extended, uint64_t *extended_starts, mf_extend_record_t *extend_records, uint64_t *unplaced,
                      mf_filter_stats_t *stats)
{
    PlaceRequest q{"alignment", true, pileup || consensus || pileup_records || ins_pile || gapped || gapped_starts || gapped_records || ext_pile || extended || extended_starts || extend_records};
    q.extend = extend; q.ext_pile = ext_pile; q.extended = extended; q.extended_starts = extended_starts; q.extend_records = extend_records;
    q.min_depth = min_depth; q.max_permille = max_permille; q.keep = keep; q.keep_bits = keep_bits; q.align = true; q.band = band;
    q.place_out = place_out; q.align_out = align_out; q.base_depth = base_depth; q.place_records = place_records;
    q.pileup = pileup; q.consensus = consensus; q.pileup_records = pileup_records; q.indels = indels; q.align_records = align_records;
    q.ins_pile = ins_pile; q.gapped = gapped; q.gapped_starts = gapped_starts; q.gapped_records = gapped_records; q.unplaced = unplaced;
    return placement_resident(ks, reads, threshold, mode, out_bits, stats, q);
}

int mf_verify(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
              uint32_t *out_bits, mf_place_t *place_out, mf_score_t *score_out, uint32_t *base_depth, mf_place_record_t *place_records,
              mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_score_record_t *score_records,
              uint64_t *unplaced, mf_filter_stats_t *stats)
{
    return mf_verify_keep(ks, reads, threshold, mode, min_depth, max_permille, MF_KEEP_PASSING, out_bits, nullptr, place_out, score_out, base_depth,
                          place_records, pileup, consensus, pileup_records, score_records, unplaced, stats);
}

} // extern "C"

// What a paired call is asked for beside its PlaceRequest: the window, the rescue, the per-set and the per-pair outputs.  score1 / score2
// are the plain call's, align1 / align2 the aligning call's (q.align); every output is optional.
struct PairRequest {
    uint32_t min_insert, max_insert; int rescue; uint32_t rescue_permille;
    uint32_t *bits1, *bits2; mf_place_t *place1, *place2; mf_score_t *score1, *score2; mf_align_t *align1, *align2;
    mf_pair_t *pairs; mf_pair_record_t *pair_records; uint64_t *pairs_none;
};

// The paired calls (include/mitofilter.h, "pairs" and "pairs with a band"): each set filtered, placed, scored -- or, for an aligning
// request, aligned -- and cut as the single-set call does it, both into ONE set of counters (the first set's cached buffers); then the
// pair kernels over both sets' pass bits and placements -- which are therefore always made on the device, asked for or not; the scores
// or alignments only where the cut can reject or the caller asks -- and the report once.
static int pairs_resident(const mf_kmerset *ks_, const mf_reads *reads1, const mf_reads *reads2, uint32_t threshold, int mode, mf_filter_stats_t *stats,
                          const PlaceRequest &q, const PairRequest &p)
{
    static_assert(sizeof(mf_pair_t) == 8 && sizeof(PairOut) == 8 && sizeof(mf_pair_record_t) == 8 * PAIR_RECORD_COUNTERS, "pair records");
    static_assert(MF_RESCUE_MAX == RESCUE_MAX && MF_PAIR_SINGLE_2 == PAIR_SINGLE_2 && MF_PAIR_RESCUED_1 == PAIR_RESCUED_1, "the kernels' constants are the header's");
    mf_kmerset *ks = const_cast<mf_kmerset *>(ks_);
    mf_reads *r1 = const_cast<mf_reads *>(reads1), *r2 = const_cast<mf_reads *>(reads2);
    const uint32_t max_permille = q.max_permille;
    // the numbers first, as the family's own check takes them; then the handles
    if (p.min_insert < 1 || p.max_insert < p.min_insert || p.max_insert > 0x7FFFFFFFu || p.max_insert - p.min_insert + 1 > MF_RESCUE_MAX)
        return fail(MF_E_ARG, "the insert window is %u .. %u: 1 <= min_insert <= max_insert < 2^31, at most %u inserts wide", p.min_insert, p.max_insert, (unsigned)MF_RESCUE_MAX);
    if (p.rescue != 0 && p.rescue != 1) return fail(MF_E_ARG, "rescue is %d: 0 or 1", p.rescue);
    if (p.rescue_permille > 1000) return fail(MF_E_ARG, "rescue_permille is %u: the cut is a number from 0 to 1000", p.rescue_permille);
    int rc = q.check(ks); if (rc) return rc;
    if (!r1 || !r2) return fail(MF_E_ARG, "NULL handle");
    if (r1 == r2) return fail(MF_E_ARG, "reads1 and reads2 are one read set: a paired call takes the two mate sets");
    if (r1->v.n_reads != r2->v.n_reads)
        return fail(MF_E_ARG, "the mate sets hold %llu and %llu reads: read i of one is the mate of read i of the other", (unsigned long long)r1->v.n_reads, (unsigned long long)r2->v.n_reads);
    if (r1->device != r2->device) return fail(MF_E_ARG, "the mate sets lie on devices %d and %d: a paired call takes both on one", r1->device, r2->device);
    mf_filter_stats_t s1{}, s2{};
    rc = filter_common(ks, r1, threshold, mode, p.bits1, nullptr, 1, stats ? &s1 : nullptr); if (rc) return rc;
    rc = filter_common(ks, r2, threshold, mode, p.bits2, nullptr, 1, stats ? &s2 : nullptr); if (rc) return rc;
    if (stats) {
        *stats = s1;
        stats->n_reads += s2.n_reads; stats->n_pass += s2.n_pass; stats->n_candidates += s2.n_candidates; stats->algorithmic_bytes += s2.algorithmic_bytes;
        stats->ms_total += s2.ms_total; stats->ms_screen += s2.ms_screen; stats->ms_mark += s2.ms_mark; stats->ms_exact += s2.ms_exact;
    }
    DevCtx *ctx, *ctx2;
    rc = get_ctx(r1->device, &ctx, r1->lane); if (rc) return rc;
    rc = get_ctx(r2->device, &ctx2, r2->lane); if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t n = r1->v.n_reads;
    const uint32_t n_rec = (uint32_t)ks->rec_len().size();
    const PlaceLayout L = q.layout(ks);
    const ReportScratch S = q.scratch(ks);
    const hipError_t e = dev_reserve(r1->d_rtot, r1->cap_rtot, L.words() * 8, false);
    if (e == hipErrorOutOfMemory && q.nomem()) return q.nomem()(L.words());
    HIPCHK(e);
    HIPCHK(dev_reserve(r1->d_rsum, r1->cap_rsum, S.sums_bytes, false));
    const hipError_t e2 = dev_reserve(r1->d_rpos, r1->cap_rpos, S.pos_bytes, false);
    if (e2 == hipErrorOutOfMemory && q.gap()) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the gapped consensus needs %llu bytes on the device", (unsigned long long)S.pos_bytes); }
    HIPCHK(e2);
    HIPCHK(hipMemsetAsync(r1->d_rtot, 0, L.words() * 8, st));
    // each set on its own stream; place_after_filter ends synchronised, so the second set adds into counters the first has left
    uint64_t listed[2] = {0, 0}, longest[2] = {0, 0};
    mf_reads *const sets[2] = {r1, r2};
    DevCtx *const ctxs[2] = {ctx, ctx2};
    ScoreOut *d_scores[2] = {nullptr, nullptr};
    AlignOut *d_aligns[2] = {nullptr, nullptr};
    for (int m = 0; m < 2 && n; m++) {
        mf_reads *r = sets[m];
        // the kernels read a placement only where the pass bit is set, and place_kernel writes every listed read's: the arrays are
        // initialised only where the caller gets them; the scores (an aligning call: the alignments) exist only where something reads them
        HIPCHK(dev_reserve(r->d_place, r->cap_place, n * sizeof(PlaceOut), true));
        if (m ? p.place2 != nullptr : p.place1 != nullptr) HIPCHK(launch_place_init(r->d_place, n, ctxs[m]->stream));
        d_scores[m] = nullptr;
        if (!q.align && ((m ? p.score2 != nullptr : p.score1 != nullptr) || max_permille < 1000)) {
            HIPCHK(dev_reserve(r->d_score, r->cap_score, n * sizeof(ScoreOut), true));
            HIPCHK(hipMemsetAsync(d_scores[m] = r->d_score, 0, n * sizeof(ScoreOut), ctxs[m]->stream));
        }
        if (q.align && ((m ? p.align2 != nullptr : p.align1 != nullptr) || max_permille < 1000)) {
            HIPCHK(dev_reserve(r->d_align, r->cap_align, n * sizeof(AlignOut), true));
            HIPCHK(hipMemsetAsync(d_aligns[m] = r->d_align, 0, n * sizeof(AlignOut), ctxs[m]->stream));
        }
        rc = place_after_filter(ks, r, L, r1->d_rtot, r->d_place, d_scores[m], &listed[m], nullptr, MF_KEEP_PASSING, d_aligns[m], &longest[m]); if (rc) return rc;
    }
    const PairLayout P(n_rec);
    std::vector<unsigned long long> h_pc(P.words(), 0);
    if (n) {
        HIPCHK(dev_reserve(r1->d_pair, r1->cap_pair, P.words() * 8 + n * sizeof(PairOut) + n * 4, true));
        unsigned long long *d_pc = r1->d_pair;
        PairOut *d_pairs = reinterpret_cast<PairOut *>(d_pc + P.words());
        uint32_t *d_list = reinterpret_cast<uint32_t *>(d_pairs + n);
        const PairWindow win{p.min_insert, p.max_insert, p.rescue_permille};
        HIPCHK(hipMemsetAsync(d_pc, 0, P.words() * 8, st));
        if (q.align) HIPCHK(launch_pair_list_aligned(r1->d_bits[r1->cur], r2->d_bits[r2->cur], r1->d_place, r2->d_place, d_aligns[0], d_aligns[1], n, max_permille, win, n_rec, d_pairs, p.rescue ? d_list : nullptr, d_pc, ctx->n_cu, st));
        else HIPCHK(launch_pair_list(r1->d_bits[r1->cur], r2->d_bits[r2->cur], r1->d_place, r2->d_place, d_scores[0], d_scores[1], n, max_permille, win, n_rec, d_pairs, p.rescue ? d_list : nullptr, d_pc, ctx->n_cu, st));
        if (p.rescue) {
            DevTables *T; rc = placement_tables(ks, r1->device, L, &T); if (rc) return rc;
            const ScoreBait bait{T->pile_words, T->pile_words_n - 1, T->pile_valid, T->pile_valid_n - 1};
            if (q.align) {
                // a target need not pass and so is on no list: the slice holds the longest read of either set
                const uint64_t max_len = std::max(longest[0], longest[1]);
                const size_t bytes = (size_t)(rescue_align_waves(n, max_len, ctx->n_cu) * align_work_words(max_len)) * 8;
                const hipError_t ew = dev_reserve(r1->d_pwork, r1->cap_pwork, bytes, false);
                if (ew == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the alignment of rescued mates of up to %llu bases needs %llu bytes on the device", (unsigned long long)max_len, (unsigned long long)bytes); }
                HIPCHK(ew);
                const RescueAlign ra{L.band, d_aligns[0], d_aligns[1], L.score_sums(r1->d_rtot), L.indel(r1->d_rtot), L.ins(r1->d_rtot), L.ext(r1->d_rtot), L.extend, r1->d_pwork, max_len};
                HIPCHK(launch_rescue_aligned(r1->v, r2->v, r1->d_bits[r1->cur], r2->d_bits[r2->cur], r1->d_place, r2->d_place, d_list, n, win, ks->k, bait, T->place_starts, n_rec, d_pairs, d_pc,
                                             L.diff(r1->d_rtot), L.cnt(r1->d_rtot), L.pile(r1->d_rtot), ra, ctx->n_cu, st));
            } else
                HIPCHK(launch_rescue(r1->v, r2->v, r1->d_bits[r1->cur], r2->d_bits[r2->cur], r1->d_place, r2->d_place, d_scores[0], d_scores[1], d_list, n, win, ks->k, bait, T->place_starts, n_rec, d_pairs, d_pc,
                                     L.diff(r1->d_rtot), L.cnt(r1->d_rtot), L.score_sums(r1->d_rtot), L.pile(r1->d_rtot), ctx->n_cu, st));
        }
        if (p.place1) HIPCHK(hipMemcpyAsync(p.place1, r1->d_place, n * sizeof(PlaceOut), hipMemcpyDeviceToHost, st));
        if (p.place2) HIPCHK(hipMemcpyAsync(p.place2, r2->d_place, n * sizeof(PlaceOut), hipMemcpyDeviceToHost, st));
        if (p.score1 && d_scores[0]) HIPCHK(hipMemcpyAsync(p.score1, d_scores[0], n * sizeof(ScoreOut), hipMemcpyDeviceToHost, st));
        if (p.score2 && d_scores[1]) HIPCHK(hipMemcpyAsync(p.score2, d_scores[1], n * sizeof(ScoreOut), hipMemcpyDeviceToHost, st));
        if (p.align1 && d_aligns[0]) HIPCHK(hipMemcpyAsync(p.align1, d_aligns[0], n * sizeof(AlignOut), hipMemcpyDeviceToHost, st));
        if (p.align2 && d_aligns[1]) HIPCHK(hipMemcpyAsync(p.align2, d_aligns[1], n * sizeof(AlignOut), hipMemcpyDeviceToHost, st));
        if (p.pairs) HIPCHK(hipMemcpyAsync(p.pairs, d_pairs, n * sizeof(PairOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_pc.data(), d_pc, P.words() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));          // (the report is told how many reads do not pass: a rescued one that did not is taken off)
    }
    if (p.pair_records)
        for (size_t j = 0; j < n_rec; j++) {
            const unsigned long long *c = h_pc.data() + PAIR_RECORD_COUNTERS * j;
            p.pair_records[j] = mf_pair_record_t{c[0], c[1], c[2], c[3], c[4], c[5]};
        }
    if (p.pairs_none) *p.pairs_none = h_pc[P.none()];
    return placement_report(ks, r1->device, st, L, r1->d_rtot, q, S, r1->d_rsum, r1->d_rpos, (n - listed[0]) + (n - listed[1]) - h_pc[P.rescued_not_passing()]);
}

extern "C" {

int mf_place_pairs(const mf_kmerset *ks, const mf_reads *reads1, const mf_reads *reads2, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
                   uint32_t min_insert, uint32_t max_insert, int rescue, uint32_t rescue_permille, uint32_t *bits1, uint32_t *bits2, mf_place_t *place1,
                   mf_place_t *place2, mf_score_t *score1, mf_score_t *score2, mf_pair_t *pairs, uint32_t *base_depth, mf_place_record_t *place_records,
                   mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_score_record_t *score_records,
                   mf_pair_record_t *pair_records, uint64_t *pairs_none, uint64_t *unplaced, mf_filter_stats_t *stats)
{
    PlaceRequest q{"pair-aware placement", true, pileup || consensus || pileup_records};
    q.min_depth = min_depth; q.max_permille = max_permille; q.base_depth = base_depth; q.place_records = place_records;
    q.pileup = pileup; q.consensus = consensus; q.pileup_records = pileup_records; q.score_records = score_records; q.unplaced = unplaced;
    const PairRequest p{min_insert, max_insert, rescue, rescue_permille, bits1, bits2, place1, place2, score1, score2, nullptr, nullptr, pairs, pair_records, pairs_none};
    return pairs_resident(ks, reads1, reads2, threshold, mode, stats, q, p);
}

int mf_align_pairs(const mf_kmerset *ks, const mf_reads *reads1, const mf_reads *reads2, uint32_t threshold, int mode, uint32_t min_depth,
                   uint32_t max_permille, uint32_t band, uint32_t extend, uint32_t min_insert, uint32_t max_insert, int rescue, uint32_t rescue_permille,
                   uint32_t *bits1, uint32_t *bits2, mf_place_t *place1, mf_place_t *place2, mf_align_t *align1, mf_align_t *align2, mf_pair_t *pairs,
                   uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records,
                   mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped, uint64_t *gapped_starts,
                   mf_gapped_record_t *gapped_records, mf_pileup_t *ext_pile, uint8_t *extended, uint64_t *extended_starts, mf_extend_record_t *extend_records,
                   mf_pair_record_t *pair_records, uint64_t *pairs_none, uint64_t *unplaced, mf_filter_stats_t *stats)
{
    PlaceRequest q{"pair-aware alignment", true, pileup || consensus || pileup_records || ins_pile || gapped || gapped_starts || gapped_records || ext_pile || extended || extended_starts || extend_records};
    q.extend = extend; q.ext_pile = ext_pile; q.extended = extended; q.extended_starts = extended_starts; q.extend_records = extend_records;
    q.min_depth = min_depth; q.max_permille = max_permille; q.align = true; q.band = band;
    q.base_depth = base_depth; q.place_records = place_records;
    q.pileup = pileup; q.consensus = consensus; q.pileup_records = pileup_records; q.indels = indels; q.align_records = align_records;
    q.ins_pile = ins_pile; q.gapped = gapped; q.gapped_starts = gapped_starts; q.gapped_records = gapped_records; q.unplaced = unplaced;
    const PairRequest p{min_insert, max_insert, rescue, rescue_permille, bits1, bits2, place1, place2, nullptr, nullptr, align1, align2, pairs, pair_records, pairs_none};
    return pairs_resident(ks, reads1, reads2, threshold, mode, stats, q, p);
}

} // extern "C"

// ------------------------------------------------------------- file level
// What filter_fastq_files_on is given to report with: after_pass runs behind every mate batch's filter pass, on the worker thread that ran
// it, before that worker's read set is filled again (mf_pipeline.h); the host pipeline hands it no read set for an empty batch.
static int hook_result(int rc, std::string &err) { if (rc != MF_OK) err = mf_thread_error(); return rc; }

// reads per record or per group: the batch's pairs, which the ingest path tallies once the pair rule has decided
struct AssignReport : PassReport {
    mf_kmerset *ks; bool by_group;
    AssignReport(mf_kmerset *ks_, bool by_group_) : PassReport(by_group_ ? ks_->n_groups() : (uint32_t)ks_->bait.rec_len.size()), ks(ks_), by_group(by_group_) {}
    int after_pass(mf_reads *R, std::vector<uint64_t> &pairs, std::string &err) override { return R ? hook_result(assign_after_filter(ks, R, nullptr, nullptr, &pairs, by_group), err) : MF_OK; }
};

// Reports that count on the device: what every mate that passes adds goes into 64-bit counters, one array per (logical) device, made and
// zeroed when a batch there first asks for it (on), shared by the device's workers and lanes (the kernels' adds are atomic), summed on
// the host at the end (fold_into).  No pairs: nothing is tallied.  A report says which tables of the set its kernels need on a device,
// how many words its array has there, and what a batch adds.
struct DeviceTotals : PassReport {
    mf_kmerset *ks;
    int (*const nomem)(size_t words);          // what a full device is reported with (null: as any failed HIP call)
    std::mutex tot_mu;
    std::map<int, unsigned long long *> tot;
    size_t n_words = 0;
    explicit DeviceTotals(mf_kmerset *ks_, int (*nomem_)(size_t) = nullptr) : PassReport(0, false), ks(ks_), nomem(nomem_) {}
    ~DeviceTotals() { release(); }
    void restart() override { release(); }
    virtual int tables(int device, DevTables *T) = 0;
    virtual size_t words(const DevTables *T) const = 0;
    virtual int add(mf_reads *R, unsigned long long *t) = 0;
    void release() { for (auto &kv : tot) if (hipSetDevice(phys(kv.first)) == hipSuccess) hipFree(kv.second); tot.clear(); }
    int on(int device, unsigned long long **out)
    {
        std::lock_guard<std::mutex> lk(tot_mu);
        auto it = tot.find(device);
        if (it != tot.end()) { *out = it->second; return MF_OK; }
        DevTables *T; int rc = build_on_device(ks, device, &T); if (rc) return rc;
        rc = tables(device, T); if (rc) return rc;
        DevCtx *ctx; rc = get_ctx(device, &ctx); if (rc) return rc;
        n_words = std::max<size_t>(words(T), 1);
        unsigned long long *p = nullptr;
        const hipError_t e = dev_malloc(&p, n_words * 8);
        if (e == hipErrorOutOfMemory && nomem) return nomem(n_words);
        HIPCHK(e);
        tot[device] = p;
        HIPCHK(hipMemsetAsync(p, 0, n_words * 8, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        *out = p;
        return MF_OK;
    }
    int after_pass(mf_reads *R, std::vector<uint64_t> &, std::string &err) override
    {
        if (!R) return MF_OK;
        unsigned long long *t = nullptr;
        int rc = on(R->device, &t);
        if (rc == MF_OK) rc = add(R, t);
        return hook_result(rc, err);
    }
    // the devices' counters summed on the host into the first listed device's, which *t0 then names
    int fold_into(int dev0, unsigned long long **t0)
    {
        int rc = on(dev0, t0); if (rc) return rc;
        if (tot.size() > 1) {
            std::vector<uint64_t> sum(n_words, 0), part(n_words);
            for (auto &kv : tot) {
                HIPCHK(hipSetDevice(phys(kv.first)));
                HIPCHK(hipMemcpy(part.data(), kv.second, n_words * 8, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < n_words; i++) sum[i] += part[i];
            }
            HIPCHK(hipSetDevice(phys(dev0)));
            HIPCHK(hipMemcpy(*t0, sum.data(), n_words * 8, hipMemcpyHostToDevice));
        }
        return MF_OK;
    }
};

// K-mer depth: the windows of every mate that passes
struct DepthTotals : DeviceTotals {
    using DeviceTotals::DeviceTotals;
    int tables(int device, DevTables *T) override { return depth_tables(ks, device, T); }
    size_t words(const DevTables *T) const override { return T->dcnt_n; }
    int add(mf_reads *R, unsigned long long *t) override { return depth_after_filter(ks, R, t); }
};

// The placement family: the footprints, record counters and (with a pile-up) bases of every mate that passes, into the layout of the
// request q, and how many mates there were and passed.  A verifying request: the placed reads are scored and cut at max_permille first.
// With a keep mode other than MF_KEEP_PASSING the batch's keep bitmap (the read set's d_keep) replaces the host copy of its pass bits
// before the ingest path's pair rule sees them (amend_bits): the reports count what they counted, the files take what is left.
struct PlaceTotals : DeviceTotals {
    const PlaceLayout L;
    const int keep;
    std::atomic<uint64_t> mates{0}, passing{0};
    PlaceTotals(mf_kmerset *ks_, const PlaceRequest &q) : DeviceTotals(ks_, q.nomem()), L(q.layout(ks_)), keep(q.keep) {}
    void restart() override { release(); mates = 0; passing = 0; }
    int tables(int device, DevTables *T) override { return placement_tables(ks, device, L, &T); }
    size_t words(const DevTables *) const override { return L.words(); }
    int add(mf_reads *R, unsigned long long *t) override
    {
        uint64_t listed = 0;
        DevCtx *ctx; int rc = get_ctx(R->device, &ctx, R->lane); if (rc) return rc;
        uint32_t *d_keep = nullptr;
        rc = keep_bitmap(R, keep, ctx->stream, &d_keep); if (rc) return rc;
        rc = place_after_filter(ks, R, L, t, nullptr, nullptr, &listed, d_keep, keep);
        if (rc == MF_OK) { mates += R->v.n_reads; passing += listed; }
        return rc;
    }
    int amend_bits(mf_reads *R, uint32_t *bits, uint64_t n, std::string &err) override
    {
        if (keep == MF_KEEP_PASSING || !R || !n) return MF_OK;
        return hook_result(copy_keep(R, bits, n), err);
    }
    static int copy_keep(mf_reads *R, uint32_t *bits, uint64_t n)
    {
        if (n != R->v.n_reads || !R->d_keep) return fail(MF_E_ARG, "the keep bitmap does not belong to this batch");
        DevCtx *ctx; const int rc = get_ctx(R->device, &ctx, R->lane); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(bits, R->d_keep, (size_t)((n + 31) / 32) * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return MF_OK;
    }
};

static int files_by_owner(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2, uint32_t threshold, int pair_mode,
                          const int *devices, int n_devices, bool by_group, uint64_t *counts, uint64_t *kept, uint64_t *total)
{
    AssignReport report(ks, by_group);
    const int rc = filter_fastq_files_on(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, &report);
    if (rc) return rc;
    std::copy(report.counts.begin(), report.counts.end(), counts);
    return MF_OK;
}

// The file-level call with a counting report, then its devices' counters summed into the first listed device's (*t0), whose context
// *ctx is: the report's last step runs once, there.
static int files_with_totals(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2, uint32_t threshold, int pair_mode,
                             const int *devices, int n_devices, uint64_t *kept, uint64_t *total, DeviceTotals &dt, unsigned long long **t0, DevCtx **ctx)
{
    int rc = filter_fastq_files_on(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, &dt);
    if (rc == MF_OK) rc = dt.fold_into(devices[0], t0);
    if (rc == MF_OK) rc = get_ctx(devices[0], ctx);
    return rc;
}

// The file-level call of the family: the counters of every mate that passes summed over the devices, then the report once, on the
// first listed device, in two temporaries of its own.
static int placement_files(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2, uint32_t threshold, int pair_mode,
                           const int *devices, int n_devices, uint64_t *kept, uint64_t *total, const PlaceRequest &q)
{
    int rc = q.check(ks); if (rc) return rc;
    PlaceTotals pt(ks, q);
    unsigned long long *t0 = nullptr; DevCtx *ctx = nullptr;
    rc = files_with_totals(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, pt, &t0, &ctx);
    if (rc) return rc;
    const ReportScratch S = q.scratch(ks);
    DevScratch tmp;
    unsigned long long *sums = nullptr; uint8_t *pos = nullptr;
    if (S.sums_bytes) HIPCHK(tmp.alloc(sums, S.sums_bytes));
    if (S.pos_bytes) {
        const hipError_t e = tmp.alloc(pos, S.pos_bytes);
        if (e == hipErrorOutOfMemory && q.gap()) { (void)hipGetLastError(); return fail(MF_E_NOMEM, "the gapped consensus needs %llu bytes on the device", (unsigned long long)S.pos_bytes); }
        HIPCHK(e);
    }
    return placement_report(ks, devices[0], ctx->stream, pt.L, t0, q, S, sums, pos, pt.mates - pt.passing);
}

extern "C" {

int mf_filter_fastq_files_by_record(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                    uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                    uint64_t *record_reads, uint64_t *kept, uint64_t *total)
{
    int rc = need_nucleotide(ks); if (rc) return rc;
    if (!record_reads) return fail(MF_E_ARG, "record_reads is NULL");
    return files_by_owner(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, false, record_reads, kept, total);
}

int mf_filter_fastq_files_by_group(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                   uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                   uint64_t *group_reads, uint64_t *kept, uint64_t *total)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    if (!group_reads) return fail(MF_E_ARG, "group_reads is NULL");
    return files_by_owner(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, true, group_reads, kept, total);
}

int mf_filter_fastq_files_depth(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                uint32_t *profile, mf_depth_record_t *records, uint64_t *kept, uint64_t *total)
{
    if (!ks) return fail(MF_E_ARG, "NULL handle");
    DepthTotals dt(ks);
    unsigned long long *t0 = nullptr; DevCtx *ctx = nullptr;
    const int rc = files_with_totals(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, dt, &t0, &ctx);
    if (rc) return rc;
    DevScratch tmp;
    DepthScratch s{nullptr, nullptr};
    HIPCHK(tmp.alloc(s.prof, DepthScratch::prof_bytes(ks)));
    HIPCHK(tmp.alloc(s.rec, DepthScratch::rec_bytes(ks)));
    return depth_report(ks, devices[0], ctx->stream, t0, s, profile, records);
}

int mf_filter_fastq_files_placed(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                 uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                 uint32_t *base_depth, mf_place_record_t *records, uint64_t *unplaced, uint64_t *kept, uint64_t *total)
{
    PlaceRequest q{"placement", false, false};
    q.base_depth = base_depth; q.place_records = records; q.unplaced = unplaced;
    return placement_files(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, q);
}

int mf_filter_fastq_files_pileup(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                 uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth,
                                 mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *records, uint64_t *unplaced,
                                 uint64_t *kept, uint64_t *total)
{
    PlaceRequest q{"the pile-up", false, true};
    q.min_depth = min_depth; q.pileup = pileup; q.consensus = consensus; q.pileup_records = records; q.unplaced = unplaced;
    return placement_files(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, q);
}

int mf_filter_fastq_files_verified_keep(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                        uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille,
                                        int keep, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
                                        mf_pileup_record_t *pileup_records, mf_score_record_t *score_records, uint64_t *unplaced, uint64_t *kept,
                                        uint64_t *total)
{
    PlaceRequest q{"verification", true, pileup || consensus || pileup_records};
    q.min_depth = min_depth; q.max_permille = max_permille; q.keep = keep; q.base_depth = base_depth; q.place_records = place_records;
    q.pileup = pileup; q.consensus = consensus; q.pileup_records = pileup_records; q.score_records = score_records; q.unplaced = unplaced;
    return placement_files(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, q);
}

int mf_filter_fastq_files_aligned(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                  uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
                                  uint32_t band, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
                                  mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records, uint64_t *unplaced,
                                  uint64_t *kept, uint64_t *total)
{
    return mf_filter_fastq_files_gapped(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, min_depth, max_permille, keep, band, base_depth,
                                        place_records, pileup, consensus, pileup_records, indels, align_records, nullptr, nullptr, nullptr, nullptr, unplaced,
                                        kept, total);
}

int mf_filter_fastq_files_gapped(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                 uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
                                 uint32_t band, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
                                 mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped,
                                 uint64_t *gapped_starts, mf_gapped_record_t *gapped_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total)
{
    return mf_filter_fastq_files_extended(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, min_depth, max_permille, keep, band, 0, base_depth,
                                          place_records, pileup, consensus, pileup_records, indels, align_records, ins_pile, gapped, gapped_starts, gapped_records,
                                          nullptr, nullptr, nullptr, nullptr, unplaced, kept, total);
}

int mf_filter_fastq_files_extended(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                   uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
                                   uint32_t band, uint32_t extend, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
                                   mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped,
                                   uint64_t *gapped_starts, mf_gapped_record_t *gapped_records, mf_pileup_t *ext_pile, uint8_t *extended,
                                   uint64_t *extended_starts, mf_extend_record_t *extend_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total)
{
    PlaceRequest q{"alignment", true, pileup || consensus || pileup_records || ins_pile || gapped || gapped_starts || gapped_records || ext_pile || extended || extended_starts || extend_records};
    q.extend = extend; q.ext_pile = ext_pile; q.extended = extended; q.extended_starts = extended_starts; q.extend_records = extend_records;
    q.min_depth = min_depth; q.max_permille = max_permille; q.keep = keep; q.align = true; q.band = band; q.base_depth = base_depth; q.place_records = place_records;
    q.pileup = pileup; q.consensus = consensus; q.pileup_records = pileup_records; q.indels = indels; q.align_records = align_records;
    q.ins_pile = ins_pile; q.gapped = gapped; q.gapped_starts = gapped_starts; q.gapped_records = gapped_records; q.unplaced = unplaced;
    return placement_files(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, kept, total, q);
}

int mf_filter_fastq_files_verified(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                   uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille,
                                   uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
                                   mf_pileup_record_t *pileup_records, mf_score_record_t *score_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total)
{
    return mf_filter_fastq_files_verified_keep(ks, fq1, fq2, out1, out2, threshold, pair_mode, devices, n_devices, min_depth, max_permille, MF_KEEP_PASSING,
                                               base_depth, place_records, pileup, consensus, pileup_records, score_records, unplaced, kept, total);
}

} // extern "C"
