// Record assignment of baited reads (gfx950, 64-wide waves).
//
//   build_owner_kernel   one thread per bait window: the window's slot in the key table, its record by a binary search over the record
//                        starts (mapped to its group when a record -> group map is given), atomicMin / atomicMax of the result into two
//                        slot-indexed arrays; owner_finish_kernel keeps the owner where both agree and marks the key shared otherwise --
//                        the same table whatever order the windows come in.
//   build_powner_kernel  the same for a protein set: one thread per residue that starts a valid window (peptide key, slot, record, group).
//   pass_list_kernel     the passing reads of a pass bitmap as a list (one atomic append per non-zero bitmap word).
//   assign_kernel        one wave per listed read, grid-stride.  Lanes take the read's windows 64 at a time: canonical key, slot,
//                        owner.  The per-read tally u_j lives in a (record, count) map held one entry per lane in registers; a
//                        ballot / readfirstlane leader loop folds the 64 lanes' owners into it, one distinct record per turn.  A read
//                        that carries unique k-mers of more than 64 records is settled exactly by repeated sweeps: a full map keeps
//                        the 64 smallest records it has seen (a record larger than all of them is skipped, the largest is evicted for
//                        a smaller newcomer), so after a sweep the map holds exact counts of the smallest records, and the next sweep
//                        starts behind them.  (The tally and the gathering of the counts are mf_tally_dev.h's, shared with mf_place.hip.)
//   passign_kernel       the same tally (assign_listed below, shared code) over the (strand, start) windows of a protein set: a lane
//                        translates its window's kp codons through a 64-entry codon table in LDS into the peptide key.
//
// k-mer depth of the bait positions (mf_depth):
//   build_rep_kernel     one thread per bait position: the slot of the valid window that starts there into pos_rep, and atomicMin of
//   build_prep_kernel    the position into rep[slot] (protein sets: the peptide key from the residues) -- rep[slot] is the smallest
//                        position whose valid window holds the key, whatever order the windows come in; rep_finish_kernel then turns
//                        pos_rep into the representative position of every valid window (DEPTH_NONE where none starts).
//   depth_kernel         one wave per listed read (grid-stride), its windows 64 at a time: key, slot, rep[slot], atomicAdd of 1 into
//   pdepth_kernel        cnt[rep].  A read drawn from the bait has consecutive windows on consecutive bait positions, so a wave's
//                        atomics fall on ~256 contiguous bytes of cnt instead of 64 hashed lines.  The window walks are the assign
//                        kernels' (NucWindows / ProtWindows), with rep in place of the owner table.  Keys that several lanes of a
//                        wave hold (low-complexity reads) are added once by count while the first pending key is one of them.
//   depth_fold_kernel    a pass's 32-bit counters into 64-bit totals (atomics: the totals of a device are shared by its lanes).
//   depth_profile_kernel one wave per item (a stretch of at most DEPTH_ITEM positions of one record): the profile from pos_rep and the
//                        totals, the record's windows / covered / sum / max reduced over the wave, one atomic of each per item.
#include "mf_tally_dev.h"
#include <algorithm>

namespace mf {

template <int KW>
__global__ void __launch_bounds__(256)
build_owner_kernel(BaitView B, const uint64_t *__restrict__ rec_start, uint32_t n_rec, const uint32_t *__restrict__ rec_group, KmerSetView S,
                   uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B.total || B.runlen[p] < (uint32_t)S.k) return;          // (runlen: valid bases from p inside its record, capped at 255 >= k)
    const uint64_t slot = table_find(S, canonical_at<KW>(B.words, p, S.k));
    if (slot == ~0ULL) return;                                          // (cannot happen: every valid window's key is in the set)
    uint32_t a = 0, b = n_rec;                                          // last record that starts at or before p (empty records start where the next does)
    while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (rec_start[m] <= p) a = m; else b = m; }
    const uint32_t o = rec_group ? rec_group[a] : a;
    atomicMin(&lo[slot], o);
    atomicMax(&hi[slot], o);
}

// protein set: one thread per residue whose run is a whole window; aa / runlen as the table builder takes them (mf_protein.hip)
__global__ void __launch_bounds__(256)
build_powner_kernel(const uint8_t *__restrict__ aa, const uint8_t *__restrict__ runlen, uint64_t total, const uint64_t *__restrict__ rec_start,
                    uint32_t n_rec, const uint32_t *__restrict__ rec_group, KmerSetView S, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total || runlen[p] < (uint32_t)S.k) return;
    uint64_t v = 0;
    for (int i = 0; i < S.k; i++) v |= (uint64_t)aa[p + i] << (5 * i);            // first residue least significant
    const uint64_t slot = table_find(S, Key<1>{v});
    if (slot == ~0ULL) return;
    uint32_t a = 0, b = n_rec;
    while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (rec_start[m] <= p) a = m; else b = m; }
    const uint32_t o = rec_group ? rec_group[a] : a;
    atomicMin(&lo[slot], o);
    atomicMax(&hi[slot], o);
}

__global__ void owner_finish_kernel(uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint64_t slots)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < slots) { const uint32_t a = lo[s]; lo[s] = a == hi[s] ? a : OWNER_SHARED; }
}

// a thread takes PL_WPT consecutive bitmap words; the workgroup reserves its place in the list with ONE atomic (same-address atomics
// serialise across the chip: one per non-zero word cost 0.18 ms on 33 M reads)
constexpr int PL_BLOCK = 256, PL_WPT = 8;
__global__ void __launch_bounds__(PL_BLOCK)
pass_list_kernel(const uint32_t *__restrict__ bits, uint64_t n_reads, uint32_t *__restrict__ list, unsigned long long *__restrict__ n_list)
{
    __shared__ uint32_t s_wave[PL_BLOCK / 64];
    __shared__ unsigned long long s_base;
    const uint64_t n_w = (n_reads + 31) / 32;
    const uint64_t w0 = ((uint64_t)blockIdx.x * PL_BLOCK + threadIdx.x) * PL_WPT;
    uint32_t v[PL_WPT], cnt = 0;
#pragma unroll
    for (int j = 0; j < PL_WPT; j++) {
        const uint64_t w = w0 + j;
        v[j] = w < n_w ? bits[w] : 0u;
        const uint64_t rem = w < n_w ? n_reads - w * 32 : 32;
        if (rem < 32) v[j] &= (1u << rem) - 1;
        cnt += __popc(v[j]);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int i = 0; i < PL_BLOCK / 64; i++) tot += s_wave[i];
        s_base = tot ? atomicAdd(n_list, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    uint64_t at = s_base + incl - cnt;
    for (int i = 0; i < wid; i++) at += s_wave[i];
#pragma unroll
    for (int j = 0; j < PL_WPT; j++)
        for (uint32_t x = v[j]; x; x &= x - 1) list[at++] = (uint32_t)((w0 + j) * 32 + (uint32_t)(__ffs(x) - 1));
}

// (the window walk of a nucleotide set, NucWindows, is mf_tally_dev.h's)

// protein set: the read's (strand, start) windows of kp codons -- starts 0 .. len - 3kp forward, then the same starts on the reverse
// strand; lut: 64 codon entries, forward residue in bits 0-4, reverse-complement residue in bits 8-12 (31: stop codon)
struct ProtWindows {
    const ReadsView &R; const KmerSetView &S; const uint32_t *__restrict__ owner; const uint32_t *lut;
    uint64_t b0 = 0, np = 0; bool hasn = false;
    __device__ ProtWindows(const ReadsView &R_, const KmerSetView &S_, const uint32_t *owner_, const uint32_t *lut_) : R(R_), S(S_), owner(owner_), lut(lut_) {}
    __device__ __forceinline__ uint64_t begin(uint32_t r)
    {
        uint64_t len;
        if (R.uniform_len) { b0 = (uint64_t)r * R.uniform_len; len = R.uniform_len; }
        else { b0 = R.offsets[r]; len = R.offsets[r + 1] - b0; }
        hasn = (R.has_n[r >> 5] >> (r & 31)) & 1u;
        const uint64_t span = 3 * (uint64_t)S.k;
        np = len >= span ? len - span + 1 : 0;
        return 2 * np;
    }
    __device__ __forceinline__ uint32_t owner_at(uint64_t w) const
    {
        const uint32_t kp = (uint32_t)S.k;
        const bool rev = w >= np;
        const uint64_t g = b0 + (rev ? w - np : w);
        if (hasn) { const uint64_t ni = npos_lower_bound(R, g); if (ni < R.n_npos && R.npos[ni] < g + 3 * (uint64_t)kp) return OWNER_SHARED; }
        const uint32_t sh = rev ? 8u : 0u;
        uint64_t key = 0;
        for (uint32_t i = 0; i < kp; i++) {
            const uint64_t bit = 2 * (g + 3 * i);
            const uint64_t wi = bit >> 5;
            const uint32_t c = alignbit(R.words[wi + 1], R.words[wi], (uint32_t)bit & 31) & 63u;
            const uint32_t res = (lut[c] >> sh) & 31u;
            if (res == 31u) return OWNER_SHARED;                           // stop codon
            key |= (uint64_t)res << (5 * (rev ? kp - 1 - i : i));           // the reverse strand's peptide runs towards lower positions
        }
        const uint64_t slot = table_find(S, Key<1>{key});
        return slot != ~0ULL ? owner[slot] : OWNER_SHARED;
    }
};

// The listed reads, one wave each (grid-stride), tallied over the windows `src` gives: the result of every read, and the counts.
template <class Src>
__device__ __forceinline__ void assign_listed(Src &src, const uint32_t *__restrict__ list, const unsigned long long *__restrict__ n_list_p, uint32_t n_rec,
                                              uint32_t *__restrict__ assign, uint64_t *__restrict__ pairs, unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t s_hist[HIST_MAX];
    GatheredCounts cnt(s_hist, counts, n_rec + 1);       // the records, then ambiguous
    cnt.hist_begin();
    const int lane = threadIdx.x & 63;
    const uint64_t n_list = *n_list_p;
    const uint64_t n_waves = (uint64_t)gridDim.x * (ASSIGN_BLOCK / 64);
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_list; i += n_waves) {
        const uint32_t r = list[i];
        const uint64_t np = src.begin(r);
        uint32_t best_cnt = 0, best_rec = ASSIGN_AMBIGUOUS; bool tie = false;
        uint32_t lo_bound = 0;                       // the records this sweep counts: lo_bound and above
        for (;;) {
            WaveTally<uint32_t> tally;
            for (uint64_t p0 = 0; p0 < np; p0 += 64) {
                const uint64_t p = p0 + (uint64_t)lane;
                uint32_t id = OWNER_SHARED;
                if (p < np) { const uint32_t o = src.owner_at(p); if (o != OWNER_SHARED && o >= lo_bound) id = o; }
                tally.add(id, lane);
            }
            tally.fold(best_cnt, best_rec, tie);
            if (!tally.overflow) break;
            lo_bound = tally.next_bound();
        }
        const uint32_t res = (best_cnt == 0 || tie) ? ASSIGN_AMBIGUOUS : best_rec;
        if (lane == 0) {
            if (assign) assign[r] = res;
            if (pairs) pairs[i] = ((uint64_t)r << 32) | res;
            cnt.bump(res == ASSIGN_AMBIGUOUS ? n_rec : res);
        }
    }
    cnt.hist_end(lane);
}

template <int KW>
__global__ void __launch_bounds__(ASSIGN_BLOCK)
assign_kernel(ReadsView R, KmerSetView S, const uint32_t *__restrict__ owner, const uint32_t *__restrict__ list,
              const unsigned long long *__restrict__ n_list_p, uint32_t n_rec, uint32_t *__restrict__ assign, uint64_t *__restrict__ pairs,
              unsigned long long *__restrict__ counts)
{
    NucWindows<KW> src(R, S, owner);
    assign_listed(src, list, n_list_p, n_rec, assign, pairs, counts);
}

__global__ void __launch_bounds__(ASSIGN_BLOCK)
passign_kernel(ReadsView R, KmerSetView S, const uint32_t *__restrict__ owner, const uint32_t *__restrict__ list,
               const unsigned long long *__restrict__ n_list_p, uint32_t n_rec, uint32_t *__restrict__ assign, uint64_t *__restrict__ pairs,
               unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t s_lut[64];
    if (threadIdx.x < 64) {              // from the filter's codon table (mf_host.cpp codon_lut_for): residue << 5 (kp - 1), reverse residue
        const uint4 e = reinterpret_cast<const uint4 *>(S.plut)[threadIdx.x];
        const uint32_t f = (uint32_t)((((uint64_t)e.y << 32) | e.x) >> (5 * (S.k - 1)));
        s_lut[threadIdx.x] = (f & 31u) | ((e.z & 31u) << 8);
    }
    // (assign_listed synchronises the workgroup before any lane reads s_lut)
    ProtWindows src(R, S, owner, s_lut);
    assign_listed(src, list, n_list_p, n_rec, assign, pairs, counts);
}

hipError_t launch_build_owner(const BaitView &B, const uint64_t *rec_start, uint32_t n_rec, const uint32_t *rec_group, const KmerSetView &S,
                              uint32_t *owner, uint32_t *hi_scratch, hipStream_t st)
{
    const uint64_t slots = S.slot_mask + 1;
    hipError_t e = hipMemsetAsync(owner, 0xFF, slots * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(hi_scratch, 0, slots * 4, st);
    if (e != hipSuccess) return e;
    if (B.total && n_rec) {
        if (S.kw == 1) hipLaunchKernelGGL(build_owner_kernel<1>, dim3(grid_of(B.total, 256)), dim3(256), 0, st, B, rec_start, n_rec, rec_group, S, owner, hi_scratch);
        else hipLaunchKernelGGL(build_owner_kernel<2>, dim3(grid_of(B.total, 256)), dim3(256), 0, st, B, rec_start, n_rec, rec_group, S, owner, hi_scratch);
    }
    hipLaunchKernelGGL(owner_finish_kernel, dim3(grid_of(slots, 256)), dim3(256), 0, st, owner, hi_scratch, slots);
    return hipGetLastError();
}

hipError_t launch_build_powner(const uint8_t *aa, const uint8_t *runlen, uint64_t total, const uint64_t *rec_start, uint32_t n_rec,
                               const uint32_t *rec_group, const KmerSetView &S, uint32_t *owner, uint32_t *hi_scratch, hipStream_t st)
{
    const uint64_t slots = S.slot_mask + 1;
    hipError_t e = hipMemsetAsync(owner, 0xFF, slots * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(hi_scratch, 0, slots * 4, st);
    if (e != hipSuccess) return e;
    if (total && n_rec)
        hipLaunchKernelGGL(build_powner_kernel, dim3(grid_of(total, 256)), dim3(256), 0, st, aa, runlen, total, rec_start, n_rec, rec_group, S, owner, hi_scratch);
    hipLaunchKernelGGL(owner_finish_kernel, dim3(grid_of(slots, 256)), dim3(256), 0, st, owner, hi_scratch, slots);
    return hipGetLastError();
}

hipError_t launch_pass_list(const uint32_t *bits, uint64_t n_reads, uint32_t *list, unsigned long long *n_list, hipStream_t st)
{
    const uint64_t n_w = (n_reads + 31) / 32;
    if (!n_w) return hipSuccess;
    hipLaunchKernelGGL(pass_list_kernel, dim3(grid_of(n_w, PL_BLOCK * PL_WPT)), dim3(PL_BLOCK), 0, st, bits, n_reads, list, n_list);
    return hipGetLastError();
}

hipError_t launch_assign(const ReadsView &R, const KmerSetView &S, const uint32_t *owner, const uint32_t *list, const unsigned long long *n_list,
                         uint32_t n_rec, uint32_t *assign, uint64_t *pairs, unsigned long long *counts, int n_cu, hipStream_t st)
{
    if (!R.n_reads) return hipSuccess;
    // the list's length is on the device: four workgroups (32 waves) a CU at most -- a few thousand flushes of the counts --, never
    // more waves than reads
    const uint64_t waves = std::min<uint64_t>((uint64_t)(n_cu > 0 ? n_cu : 1) * 32, R.n_reads);
    const unsigned grid = grid_of(waves, ASSIGN_BLOCK / 64);
    if (S.prot) hipLaunchKernelGGL(passign_kernel, dim3(grid), dim3(ASSIGN_BLOCK), 0, st, R, S, owner, list, n_list, n_rec, assign, pairs, counts);
    else if (S.kw == 1) hipLaunchKernelGGL(assign_kernel<1>, dim3(grid), dim3(ASSIGN_BLOCK), 0, st, R, S, owner, list, n_list, n_rec, assign, pairs, counts);
    else hipLaunchKernelGGL(assign_kernel<2>, dim3(grid), dim3(ASSIGN_BLOCK), 0, st, R, S, owner, list, n_list, n_rec, assign, pairs, counts);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------ k-mer depth
template <int KW>
__global__ void __launch_bounds__(256)
build_rep_kernel(BaitView B, KmerSetView S, uint32_t *__restrict__ rep, uint32_t *__restrict__ pos_rep)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B.total) return;
    uint64_t slot = ~0ULL;
    if (B.runlen[p] >= (uint32_t)S.k) slot = table_find(S, canonical_at<KW>(B.words, p, S.k));
    if (slot == ~0ULL) { pos_rep[p] = DEPTH_NONE; return; }
    pos_rep[p] = (uint32_t)slot;
    atomicMin(&rep[slot], (uint32_t)p);
}

__global__ void __launch_bounds__(256)
build_prep_kernel(const uint8_t *__restrict__ aa, const uint8_t *__restrict__ runlen, uint64_t total, KmerSetView S, uint32_t *__restrict__ rep,
                  uint32_t *__restrict__ pos_rep)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    uint64_t slot = ~0ULL;
    if (runlen[p] >= (uint32_t)S.k) {
        uint64_t v = 0;
        for (int i = 0; i < S.k; i++) v |= (uint64_t)aa[p + i] << (5 * i);
        slot = table_find(S, Key<1>{v});
    }
    if (slot == ~0ULL) { pos_rep[p] = DEPTH_NONE; return; }
    pos_rep[p] = (uint32_t)slot;
    atomicMin(&rep[slot], (uint32_t)p);
}

// by_slot: every key counts in a counter of its own slot (rep[slot] = slot) -- the scattered form, kept to measure against
__global__ void rep_finish_kernel(uint32_t *__restrict__ rep, uint64_t slots, uint32_t *__restrict__ pos_rep, uint64_t total, int by_slot)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (by_slot && i < slots) rep[i] = (uint32_t)i;
    if (i < total) { const uint32_t s = pos_rep[i]; if (s != DEPTH_NONE) pos_rep[i] = by_slot ? s : rep[s]; }
}

constexpr int DEPTH_BLOCK = 512;

// The windows of the listed reads, one wave a read: one atomic add per window whose key the bait holds
template <class Src, class Cnt>
__device__ __forceinline__ void depth_listed(Src &src, const uint32_t *__restrict__ list, const unsigned long long *__restrict__ n_list_p, Cnt *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const uint64_t n_list = *n_list_p;
    const uint64_t n_waves = (uint64_t)gridDim.x * (DEPTH_BLOCK / 64);
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_list; i += n_waves) {
        const uint64_t np = src.begin(list[i]);
        for (uint64_t p0 = 0; p0 < np; p0 += 64) {
            const uint64_t p = p0 + (uint64_t)lane;
            uint32_t o = p < np ? src.owner_at(p) : OWNER_SHARED;
            // A run of one key (a microsatellite, poly-A) puts the wave's atomics on a few addresses, and same-address atomics
            // serialise across the chip (100 ms a pass on 2 % microsatellite reads): while the first pending key is held by several
            // lanes, one lane adds their count.  A read drawn from the bait leaves after one turn (its first key is unique).
            uint64_t pend = __ballot(o != OWNER_SHARED);
            for (int turn = 0; pend && turn < 8; turn++) {
                const uint32_t L = __builtin_amdgcn_readfirstlane(__shfl(o, (int)(__ffsll((long long)pend) - 1)));
                const uint64_t same = __ballot(o == L);
                if (__popcll(same) == 1) break;
                if ((uint64_t)lane == (uint64_t)(__ffsll((long long)same) - 1)) atomicAdd(&cnt[L], (Cnt)__popcll(same));
                if (o == L) o = OWNER_SHARED;
                pend &= ~same;
            }
            if (o != OWNER_SHARED) atomicAdd(&cnt[o], (Cnt)1);
        }
    }
}

template <int KW, class Cnt>
__global__ void __launch_bounds__(DEPTH_BLOCK)
depth_kernel(ReadsView R, KmerSetView S, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ list,
             const unsigned long long *__restrict__ n_list_p, Cnt *__restrict__ cnt)
{
    NucWindows<KW> src(R, S, rep);
    depth_listed(src, list, n_list_p, cnt);
}

template <class Cnt>
__global__ void __launch_bounds__(DEPTH_BLOCK)
pdepth_kernel(ReadsView R, KmerSetView S, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ list,
              const unsigned long long *__restrict__ n_list_p, Cnt *__restrict__ cnt)
{
    __shared__ uint32_t s_lut[64];
    if (threadIdx.x < 64) {              // (as passign_kernel)
        const uint4 e = reinterpret_cast<const uint4 *>(S.plut)[threadIdx.x];
        const uint32_t f = (uint32_t)((((uint64_t)e.y << 32) | e.x) >> (5 * (S.k - 1)));
        s_lut[threadIdx.x] = (f & 31u) | ((e.z & 31u) << 8);
    }
    __syncthreads();
    ProtWindows src(R, S, rep, s_lut);
    depth_listed(src, list, n_list_p, cnt);
}

__global__ void __launch_bounds__(256)
depth_fold_kernel(const uint32_t *__restrict__ cnt, uint64_t n, unsigned long long *__restrict__ tot)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const uint32_t c = cnt[i]; if (c) atomicAdd(&tot[i], (unsigned long long)c); }
}

__global__ void __launch_bounds__(64)
depth_profile_kernel(const DepthItem *__restrict__ items, const uint32_t *__restrict__ pos_rep, const unsigned long long *__restrict__ tot,
                     uint32_t *__restrict__ profile, unsigned long long *__restrict__ rec)
{
    const DepthItem it = items[blockIdx.x];
    unsigned long long w = 0, cov = 0, sum = 0, mx = 0;
    for (uint32_t i = threadIdx.x; i < it.len; i += 64) {
        const uint64_t p = it.begin + i;
        const uint32_t r = pos_rep[p];
        uint32_t out = DEPTH_NONE;
        if (r != DEPTH_NONE) {
            const unsigned long long d = tot[r];
            w++; cov += d != 0; sum += d; mx = d > mx ? d : mx;
            out = d < DEPTH_CLAMP ? (uint32_t)d : DEPTH_CLAMP;
        }
        if (profile) profile[p] = out;
    }
    if (!rec) return;
    w = wave_sum_u64(w); cov = wave_sum_u64(cov); sum = wave_sum_u64(sum); mx = wave_max_u64(mx);
    if (threadIdx.x == 0 && w) {
        unsigned long long *o = rec + 4 * (uint64_t)it.rec;
        atomicAdd(&o[0], w); atomicAdd(&o[1], cov); atomicAdd(&o[2], sum); atomicMax(&o[3], mx);
    }
}

hipError_t launch_build_depth(const BaitView &B, const uint8_t *aa, const KmerSetView &S, uint32_t *rep, uint32_t *pos_rep, bool by_slot,
                              hipStream_t st)
{
    const uint64_t slots = S.slot_mask + 1, total = B.total;
    hipError_t e = hipMemsetAsync(rep, 0xFF, slots * 4, st);
    if (e != hipSuccess) return e;
    if (total) {
        if (S.prot) hipLaunchKernelGGL(build_prep_kernel, dim3(grid_of(total, 256)), dim3(256), 0, st, aa, B.runlen, total, S, rep, pos_rep);
        else if (S.kw == 1) hipLaunchKernelGGL(build_rep_kernel<1>, dim3(grid_of(total, 256)), dim3(256), 0, st, B, S, rep, pos_rep);
        else hipLaunchKernelGGL(build_rep_kernel<2>, dim3(grid_of(total, 256)), dim3(256), 0, st, B, S, rep, pos_rep);
    }
    const uint64_t n = std::max<uint64_t>(by_slot ? slots : 0, total);
    if (n) hipLaunchKernelGGL(rep_finish_kernel, dim3(grid_of(n, 256)), dim3(256), 0, st, rep, slots, pos_rep, total, by_slot ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_depth_count(const ReadsView &R, const KmerSetView &S, const uint32_t *rep, const uint32_t *list, const unsigned long long *n_list,
                              uint32_t *cnt32, unsigned long long *cnt64, int n_cu, hipStream_t st)
{
    if (!R.n_reads) return hipSuccess;
    const uint64_t waves = std::min<uint64_t>((uint64_t)(n_cu > 0 ? n_cu : 1) * 32, R.n_reads);
    const unsigned grid = grid_of(waves, DEPTH_BLOCK / 64);
    if (cnt64) {
        if (S.prot) hipLaunchKernelGGL(pdepth_kernel<unsigned long long>, dim3(grid), dim3(DEPTH_BLOCK), 0, st, R, S, rep, list, n_list, cnt64);
        else if (S.kw == 1) hipLaunchKernelGGL((depth_kernel<1, unsigned long long>), dim3(grid), dim3(DEPTH_BLOCK), 0, st, R, S, rep, list, n_list, cnt64);
        else hipLaunchKernelGGL((depth_kernel<2, unsigned long long>), dim3(grid), dim3(DEPTH_BLOCK), 0, st, R, S, rep, list, n_list, cnt64);
    } else {
        if (S.prot) hipLaunchKernelGGL(pdepth_kernel<uint32_t>, dim3(grid), dim3(DEPTH_BLOCK), 0, st, R, S, rep, list, n_list, cnt32);
        else if (S.kw == 1) hipLaunchKernelGGL((depth_kernel<1, uint32_t>), dim3(grid), dim3(DEPTH_BLOCK), 0, st, R, S, rep, list, n_list, cnt32);
        else hipLaunchKernelGGL((depth_kernel<2, uint32_t>), dim3(grid), dim3(DEPTH_BLOCK), 0, st, R, S, rep, list, n_list, cnt32);
    }
    return hipGetLastError();
}

hipError_t launch_depth_fold(const uint32_t *cnt32, uint64_t n, unsigned long long *tot, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(depth_fold_kernel, dim3(grid_of(n, 256)), dim3(256), 0, st, cnt32, n, tot);
    return hipGetLastError();
}

hipError_t launch_depth_profile(const DepthItem *items, uint32_t n_items, const uint32_t *pos_rep, const unsigned long long *tot, uint32_t *profile,
                                unsigned long long *rec, hipStream_t st)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(depth_profile_kernel, dim3(n_items), dim3(64), 0, st, items, pos_rep, tot, profile, rec);
    return hipGetLastError();
}

} // namespace mf
