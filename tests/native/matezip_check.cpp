// MateZip (mf_pl_stages.h) fed from two threads, as the readers feed it: every mate's records arrive in batches of the sizes
// given on the command line, the record's index in its file written into its header length.
//   matezip_check SIZES1 SIZES2|- [SEED]     SIZES: comma-separated batch sizes, "" for a mate without a batch; "-": single end
// prints one line "n first1 first2 index1 index2" per pair batch (index: the file index of the batch's first record of that mate)
// after checking that the n records of both mates carry consecutive indices; the feeders sleep now and then (SEED).
#include "mf_pl_stages.h"
#include <chrono>

static std::vector<uint64_t> sizes(const char *s)
{
    std::vector<uint64_t> v;
    for (const char *p = s; *p;) { char *e; v.push_back(strtoull(p, &e, 10)); p = *e ? e + 1 : e; }
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const int nm = strcmp(argv[2], "-") ? 2 : 1;
    const unsigned seed = argc > 3 ? (unsigned)atoi(argv[3]) : 0;
    mf::Channel<mf::MatePtr> q_read[2] = {mf::Channel<mf::MatePtr>(2), mf::Channel<mf::MatePtr>(2)};
    auto pool = std::make_shared<mf::Pool<mf::MateBatch>>();
    std::vector<std::thread> feeders;
    for (int m = 0; m < nm; m++)
        feeders.emplace_back([&, m] {
            uint32_t index = 0; unsigned c = seed * 7919u + (unsigned)m;
            for (const uint64_t n : sizes(argv[1 + m])) {
                auto b = pool->get();
                b->recs.resize(n);
                for (uint64_t i = 0; i < n; i++) b->recs[i] = mf::FqRec{nullptr, nullptr, nullptr, index++, 0, 0};
                c = c * 1664525u + 1013904223u;
                if (seed && (c >> 28) < 3) std::this_thread::sleep_for(std::chrono::microseconds((c >> 16) % 700));
                if (!q_read[m].push(b)) break;
            }
            q_read[m].finish();
        });
    mf::MateZip zip{q_read, nm};
    uint64_t next[2] = {0, 0};
    for (;;) {
        mf::ZipBatch b;
        if (!zip.next(b)) break;
        for (int m = 0; m < nm; m++)
            for (uint64_t i = 0; i < b.n; i++)
                if (b.recs(m)[i].hl != next[m] + i) { printf("mate %d: record %llu where %llu belongs\n", m + 1, (unsigned long long)b.recs(m)[i].hl, (unsigned long long)(next[m] + i)); return 1; }
        printf("%llu %llu %llu %llu %llu\n", (unsigned long long)b.n, (unsigned long long)b.first[0], (unsigned long long)b.first[1], (unsigned long long)next[0], (unsigned long long)next[1]);
        for (int m = 0; m < nm; m++) next[m] += b.n;
    }
    for (auto &q : q_read) q.abort();          // (as the pipelines do: a feeder may still be pushing past the end of the shorter mate)
    for (auto &t : feeders) t.join();
    return 0;
}
