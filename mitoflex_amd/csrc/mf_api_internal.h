// Internals of mf_api.cpp that the device ingest path (mf_devingest.cpp) and the reports (mf_report.cpp) share: device contexts, the
// k-mer set and read-set handles, the filter call and the file-level worker.  Not part of the C ABI.
#pragma once
#include "../../include/mitofilter.h"
#include "mf_common.h"
#include "mf_host.h"
#include "mf_kernels.h"
#include "mf_assign.h"
#include "mf_place.h"
#include "mf_align_launch.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// stream2: finish kernels of pipelined passes (stream4: those of every other pass when the finish kernels are what a pass waits for); stream3: every other screen
struct DevCtx { int device = -1; hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr, stream4 = nullptr; int n_cu = 0; };

int fail(int code, const char *fmt, ...);               // sets the thread's error message, returns code
const std::string &mf_thread_error();
int phys(int device);                                   // logical -> physical device (MF_FAKE_DEVICES)
int get_ctx(int device, DevCtx **out, int lane = 0);
#define HIPCHK(call)                                                                                  \
    do { hipError_t e_ = (call);                                                                      \
         if (e_ != hipSuccess) return fail(MF_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// The device ingest path keeps device buffers of earlier calls in a pool per device (mf_devingest.cpp).  Memory that sits there idle must
// never make another allocation of this library fail: release_cached_device_memory() gives the current device's idle pool buffers (and, with
// all = true, every cache of every device: pool, consumers' scratch and read sets, pinned staging) back to the runtime; dev_malloc() is
// hipMalloc that calls it and tries once more when the device is full.  Returns the bytes released.
namespace mf { size_t release_cached_device_memory(bool all); }
inline hipError_t dev_malloc(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        if (mf::release_cached_device_memory(false)) e = hipMalloc(p, bytes);
        if (e != hipSuccess) (void)hipGetLastError();
    }
    return e;
}
template <class T> inline hipError_t dev_malloc(T **p, size_t bytes) { return dev_malloc(reinterpret_cast<void **>(p), bytes); }

// grow a device buffer to at least `bytes` (with some slack when it is being re-used)
template <class T> inline hipError_t dev_reserve(T *&p, size_t &cap, size_t bytes, bool slack)
{
    if (bytes <= cap && p) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    const size_t want = slack ? bytes + bytes / 4 + 4096 : (bytes ? bytes : 16);
    hipError_t e = dev_malloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
}


// ------------------------------------------------------------------ kmerset
struct DevTables {
    uint64_t *keys = nullptr;
    uint32_t *bloom = nullptr, *stab = nullptr, *kbloom = nullptr, *kbloom_co = nullptr, *plut = nullptr;    // kbloom_co: own allocation only when it differs from kbloom
    uint32_t *front2 = nullptr, *front3 = nullptr, *pre = nullptr;      // bait-sized fronts of the large-bait screen (front_mode 1 .. 4); mode 4's one-bit LDS table
    mf::KmerSetView view{};
    uint64_t n_keys = 0, n_smers = 0;
    uint32_t *owner = nullptr;          // record owner of every slot of `keys` (mf_assign.h), built by the first call that asks for it
    uint32_t *gowner = nullptr;         // group owner of every slot for the set's current grouping, likewise (freed when the set is regrouped)
    // k-mer depth (mf_depth), built by the first depth call: representative position of every slot, of every bait position's window, and
    // the profile kernel's work items; dcnt_n counters a pass (the positions, or the slots under depth_index=1)
    uint32_t *rep = nullptr, *pos_rep = nullptr; mf::DepthItem *ditems = nullptr; uint32_t n_ditems = 0; uint64_t dcnt_n = 0;
    // placement (mf_place), built by the first placement call: the anchor of every slot and the record starts (R + 1) the kernels read
    mf::Anchor *anchor = nullptr; uint64_t *place_starts = nullptr; bool place_built = false;
    // pile-up (mf_pileup), kept by the first pile-up call: the bait's packed bases and run lengths, which the call kernel reads, and the
    // bait's validity one bit a position, which the verifying placement reads beside the bases (pile_words_n / pile_valid_n words, each
    // padded by one)
    uint32_t *pile_words = nullptr; uint8_t *pile_runlen = nullptr; uint32_t *pile_valid = nullptr; bool pile_built = false;
    uint64_t pile_words_n = 0, pile_valid_n = 0;
    // frees one table / every table (the current device is the tables')
    template <class T> static hipError_t drop(T *&p) { const hipError_t e = hipFree(p); p = nullptr; return e; }
    void release()
    {
        drop(keys); drop(bloom); drop(stab); drop(kbloom); drop(kbloom_co); drop(plut); drop(front2); drop(front3); drop(pre);
        drop(owner); drop(gowner); drop(rep); drop(pos_rep); drop(ditems);
        drop(anchor); drop(place_starts); place_built = false;
        drop(pile_words); drop(pile_runlen); drop(pile_valid); pile_built = false;
    }
};
struct mf_kmerset {
    int k = 0, kw = 1;
    int kind = MF_KIND_NUCLEOTIDE, genetic_code = 0;   // protein sets: k = residues per key, reads translated with genetic_code
    mf::ProtBaitHost pbait;
    uint32_t codon_lut[256] = {0};
    bool kb_in_lds = true;
    mf::BaitHost bait;
    uint64_t n_windows = 0, slots = 0;
    mf::ScreenGeom geom{0, 0};
    uint32_t bloom_log2w = 0, stage2_log2w = 0, stab_slots = 0, kb_log2w = 0;
    uint32_t front_mode = 0, f2_log2b = 0, f3_log2b = 0, pre_log2w = 0;
    int canon = 0;              // != 0: the screen's tables hold one canonical key per bait s-mer (mf::KmerSetView::canon: 1 sixteen-base samples, 2 shorter)
    bool s8_finish = false;     // a stride-8 set whose threshold-1 passes go through screen + finish (baits beyond ~20 kbp)
    size_t screen_words() const { return ((size_t)1 << bloom_log2w) + ((size_t)1 << stage2_log2w); }
    // grouping of the records (mf_kmerset_group_records): empty rec_group = identity (each record its own group, named after it)
    std::vector<uint32_t> rec_group;
    std::vector<std::string> group_names;
    std::mutex mu;
    std::map<int, DevTables> dev;
    const std::vector<std::string> &names() const { return kind == MF_KIND_PROTEIN ? pbait.names : bait.names; }
    uint32_t n_records() const { return (uint32_t)names().size(); }
    uint32_t n_groups() const { return rec_group.empty() ? n_records() : (uint32_t)group_names.size(); }
    const std::string &group_name(uint64_t i) const { return rec_group.empty() ? names()[i] : group_names[i]; }
    const std::vector<uint64_t> &rec_len() const { return kind == MF_KIND_PROTEIN ? pbait.rec_len : bait.rec_len; }
    uint64_t positions() const { return kind == MF_KIND_PROTEIN ? pbait.total : bait.total; }       // bases / residues of all records
};

// device temporaries of one build: released on every exit path
struct DevScratch {
    std::vector<void *> bufs;
    template <class T> hipError_t alloc(T *&p, size_t bytes) { hipError_t e = dev_malloc(&p, bytes); if (e == hipSuccess) bufs.push_back(p); return e; }
    template <class T> T *release(T *p) { bufs.erase(std::remove(bufs.begin(), bufs.end(), (void *)p), bufs.end()); return p; }     // p outlives the build
    ~DevScratch() { for (void *p : bufs) hipFree(p); }
};
// the tables of a set on `device`, built by the first call that asks for them
int build_on_device(mf_kmerset *ks, int device, DevTables **out);
int depth_index_option();          // the "depth_index" option as it is set now (mf_set_option)

// Buffer sets a pipelined pass rotates through.  (Round 2 measured nothing from a third; since the finish kernels of two-word keys run on two streams and
// outlast a screen, it is worth 4 % of a pass for them: profiles/r06/n_three_sets.txt -- one-word keys keep to two, mf_api.cpp enqueue_pass.  A fourth adds nothing.)
#ifndef MF_NSETS
#define MF_NSETS 3
#endif
constexpr int NSETS = MF_NSETS;
struct mf_reads {
    int device = 0, lane = 0;     // lane: which of the device's contexts (streams) this read set works on
    mf::ReadsView v{};
    uint32_t *d_words = nullptr; uint64_t *d_offsets = nullptr, *d_npos = nullptr;
    uint32_t *d_has_n = nullptr, *d_hits = nullptr, *d_npos_blk = nullptr; uint64_t *d_off_blk = nullptr;
    // Threshold-1 passes (screen_kernel + finish_kernel) are pipelined: the finish kernel of pass i runs on a second stream
    // under the screen kernel of pass i + 1, the way consecutive batches of a file do.  What a pass writes therefore
    // exists NSETS times and rotates: record lists, result bitmap, tally buffer.  `cur` holds the latest result.
    uint32_t *d_cand[NSETS] = {}, *d_bits[NSETS] = {};
    void *d_recs[NSETS] = {}; uint32_t *d_rec_counts[NSETS] = {};     // stage-1 positive records (screen -> finish / mark)
    unsigned long long *d_counters[NSETS] = {};     // a tally block each (mf::TallyLayout), in pinned HOST memory: the kernels store their pair there directly and a call ends without a device-to-host copy
    hipEvent_t ev_screen[NSETS] = {}, ev_finish[NSETS] = {};          // ordering between the two streams
    hipEvent_t ev_call[2] = {};                                       // begin / end of a call's passes
    bool cand_clean[NSETS] = {}, sample_pass = false;     // sample_pass: the latest pass was a screen + finish one
    int tally_regions = 1;      // the regions of its tally block the latest pass wrote (PassPlan::tally_regions): the others hold what earlier passes left
    mf::PassFeedback fb;        // what the last call's tallies say about the input (mf_passplan.h)
    int cur = 0, flip = 0;      // flip: parity of the pipelined passes enqueued so far (which of two streams a pass's screen / finish kernels take)
    unsigned long long *tally_override = nullptr;       // set per pass by filter_common when every pass's tally is wanted
    size_t bitmap_bytes = 0;
    // record assignment (mf_assign and the file-level call by record): the passing reads as a list, their records, the counters
    uint32_t *d_alist = nullptr, *d_assign = nullptr; uint64_t *d_apairs = nullptr; unsigned long long *d_acnt = nullptr;
    size_t cap_alist = 0, cap_assign = 0, cap_apairs = 0, cap_acnt = 0;
    // the reports of mf_depth and of the placement family: d_rtot the call's 64-bit totals; d_rsum its 64-bit record sums and the work
    // words of its report kernels; d_rpos what it holds per position (mf_depth: 32-bit counters, then the profile; the placement family:
    // the sections of ReportScratch, mf_placelayout.h, in both)
    unsigned long long *d_rtot = nullptr, *d_rsum = nullptr; void *d_rpos = nullptr;
    size_t cap_rtot = 0, cap_rsum = 0, cap_rpos = 0;
    uint32_t *rpos_u32() const { return static_cast<uint32_t *>(d_rpos); }
    mf::PlaceOut *d_place = nullptr; size_t cap_place = 0;          // mf_place's per-read results
    mf::ScoreOut *d_score = nullptr; size_t cap_score = 0;          // mf_verify's per-read scores
    uint32_t *d_keep = nullptr; size_t cap_keep = 0;                // the keep bitmap of a verifying call with a keep mode: laid out like d_bits
    mf::AlignOut *d_align = nullptr; size_t cap_align = 0;          // mf_align's per-read alignments
    unsigned long long *d_awork = nullptr; size_t cap_awork = 0;    // ... and its kernel's work memory, a slice a wave (mf_align_launch.h)
    unsigned long long *d_pair = nullptr; size_t cap_pair = 0;      // mf_place_pairs (on the first set): the pair counters, the per-pair results, the rescue list
    unsigned long long *d_pwork = nullptr; size_t cap_pwork = 0;    // mf_align_pairs (on the first set): the aligning rescue's work memory, a slice a wave over the longer set's longest read
    // capacities (bytes), so that a handle can be refilled batch after batch without touching the allocator
    size_t cap_words = 0, cap_offsets = 0, cap_npos = 0, cap_bitmap = 0, cap_recs = 0, cap_rec_counts = 0, cap_hits = 0, cap_npos_blk = 0, cap_off_blk = 0;
};


void reads_release(mf_reads *r);
// Device buffers of a read set that the caller fills on the device: packed words (padded, the tail behind n_words zeroed),
// offsets (n_reads + 1, unless uniform_len), room for npos_cap invalid positions.
int reads_reserve(mf_reads *r, bool reuse, uint64_t n_words, uint64_t n_reads, uint32_t uniform_len, uint64_t npos_cap, DevCtx *ctx);
// ... and what follows once words / offsets / npos are in place (index over the invalid positions, bitmaps, record lists).
// Ends synchronised.
int reads_finish(mf_reads *r, bool reuse, uint64_t n_words, uint64_t n_reads, uint64_t total_bases, uint32_t uniform_len, uint64_t n_npos, DevCtx *ctx);
// one or more passes of the filter over a resident read set; out_bits / hits_out may be null (the result stays in r->d_bits[r->cur])
int filter_common(const mf_kmerset *ks, const mf_reads *reads, uint32_t thr, int mode, uint32_t *out_bits, uint32_t *hits_out, int steps,
                  mf_filter_stats_t *stats, uint64_t *pass_per_step = nullptr);
// the file-level call on a list of (logical) devices; report: what it reports on the reads that pass (mf_pipeline.h), or null
namespace mf { struct PassReport; }
int filter_fastq_files_on(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                          uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint64_t *kept, uint64_t *total, mf::PassReport *report);
