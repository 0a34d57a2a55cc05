// The quality filter's decisions (mf_qualdecide.h) and their run over a batch on several threads (mf_pl_stages.h), called
// directly: no reader, no channel, no device.  Commands are read from the file named on the command line, one a line, strings
// in hex ("-": empty); every command prints one line.
//   cut NM START END N  + N lines "h s q [h2 s2 q2]"  -> "cut FIRST_BAD" and, per record and mate, " s q" as they are afterwards
//   drop NM SL1 QL1 N1 N2 B1 B2 NS LIMIT_BITS           -> "drop 0|1"          (LIMIT_BITS: the f32's bits in hex)
//   take TRIM BUDGET HAVE_ALIVE HAVE_DUP N + N lines "alive dup sl"  -> "take KEEP-STRING kept stop budget"
//   par THREADS N NM START BAD...                       -> "par FIRST_BAD"     (N good records; those at BAD... are made bad: odd
//                                                          ones by a sequence of mate NM shorter than START, even ones by a lone 0x80)
#include "mf_pl_stages.h"
#include <fstream>
#include <sstream>
#include <string>

static std::string unhex(const std::string &h)
{
    std::string o;
    if (h == "-") return o;
    for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return o;
}
static std::string hex(const char *p, uint32_t n)
{
    if (!n) return "-";
    static const char *d = "0123456789abcdef"; std::string o;
    for (uint32_t i = 0; i < n; i++) { o.push_back(d[(unsigned char)p[i] >> 4]); o.push_back(d[p[i] & 15]); }
    return o;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line); std::string cmd; ls >> cmd;
        if (cmd == "cut") {
            int nm; mf::QualParams P; uint64_t n; ls >> nm >> P.start >> P.end >> n;
            std::vector<std::vector<char>> text((size_t)n * 6);          // every string in a buffer of exactly its size: ASan sees a read past its end
            std::vector<mf::FqRec> recs[2]; recs[0].resize(n); recs[1].resize(n);
            for (uint64_t i = 0; i < n; i++) {
                std::getline(in, line); std::istringstream rs(line);
                for (int m = 0; m < nm; m++) {
                    std::string f[3]; rs >> f[0] >> f[1] >> f[2];
                    for (int k = 0; k < 3; k++) { const std::string u = unhex(f[k]); text[i * 6 + m * 3 + k].assign(u.begin(), u.end()); }
                    const std::vector<char> *t = &text[i * 6 + m * 3];
                    recs[m][i] = mf::FqRec{t[0].data(), t[1].data(), t[2].data(), (uint32_t)t[0].size(), (uint32_t)t[1].size(), (uint32_t)t[2].size()};
                }
            }
            mf::FqRec *const mrec[2] = {recs[0].data(), nm == 2 ? recs[1].data() : nullptr};
            printf("cut %llu", (unsigned long long)mf::qual_check_cut(mrec, nm, 0, n, P));
            for (uint64_t i = 0; i < n; i++) for (int m = 0; m < nm; m++) printf(" %s %s", hex(recs[m][i].s, recs[m][i].sl).c_str(), hex(recs[m][i].q, recs[m][i].ql).c_str());
            printf("\n");
        } else if (cmd == "drop") {
            int nm; mf::FqRec r1{}; uint32_t nc[2], bc[2]; uint64_t ns; std::string bits;
            ls >> nm >> r1.sl >> r1.ql >> nc[0] >> nc[1] >> bc[0] >> bc[1] >> ns >> bits;
            const uint32_t u = (uint32_t)strtoul(bits.c_str(), nullptr, 16); float limit; memcpy(&limit, &u, 4);
            printf("drop %d\n", mf::qual_drop(nm, r1, nc, bc, ns, limit) ? 1 : 0);
        } else if (cmd == "take") {
            uint64_t trim, budget, n; int have_alive, have_dup; ls >> trim >> budget >> have_alive >> have_dup >> n;
            std::vector<uint8_t> alive(n), dup(n), keep(n ? n : 1, 0); std::vector<mf::FqRec> recs(n);
            for (uint64_t i = 0; i < n; i++) { std::getline(in, line); std::istringstream rs(line); int a, d; rs >> a >> d >> recs[i].sl; alive[i] = (uint8_t)a; dup[i] = (uint8_t)d; }
            const mf::QualTake t = mf::qual_take(have_alive ? alive.data() : nullptr, have_dup ? dup.data() : nullptr, recs.data(), n, trim, budget, keep.data());
            std::string ks; for (uint64_t i = 0; i < n; i++) ks.push_back(keep[i] ? '1' : '0');
            printf("take %s %llu %d %llu\n", n ? ks.c_str() : "-", (unsigned long long)t.kept, t.stop ? 1 : 0, (unsigned long long)budget);
        } else if (cmd == "par") {
            int threads, nm; uint64_t n; mf::QualParams P; ls >> threads >> n >> nm >> P.start;
            const std::string h = "@r", s(12, 'A'), q(12, 'I'), short_s(P.start ? P.start - 1 : 0, 'C'), lone = "AC\x80GTACGTACGT";
            std::vector<mf::FqRec> recs[2];
            for (int m = 0; m < nm; m++) recs[m].assign(n, mf::FqRec{h.data(), s.data(), q.data(), (uint32_t)h.size(), (uint32_t)s.size(), (uint32_t)q.size()});
            for (uint64_t b; ls >> b;) {
                mf::FqRec &r = recs[nm - 1][b];
                if (b & 1) { r.s = short_s.data(); r.sl = (uint32_t)short_s.size(); } else { r.s = lone.data(); r.sl = (uint32_t)lone.size(); }
            }
            mf::FqRec *const mrec[2] = {recs[0].data(), nm == 2 ? recs[1].data() : nullptr};
            printf("par %llu\n", (unsigned long long)mf::qual_check_cut_batch(mrec, nm, n, P, threads));
        } else if (!cmd.empty()) return 3;
    }
    return 0;
}
