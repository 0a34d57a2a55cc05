// Device helpers that the record-assignment kernels (mf_assign.hip) and the placement kernels (mf_place.hip) share: wave reductions, the
// window walk of a nucleotide read, the per-wave (key, count) tally with its leader loop, and the per-workgroup gathering of counters
// that many reads bump.  64-wide waves.
#pragma once
#include "mf_assign.h"
#include "mf_keys_dev.h"

namespace mf {

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_max_u32(v); }
__device__ __forceinline__ uint64_t wave_max(uint64_t v) { return wave_max_u64(v); }
// lane src's value, in scalar registers
__device__ __forceinline__ uint32_t wave_pick(uint32_t v, int src) { return __builtin_amdgcn_readfirstlane(__shfl(v, src)); }
__device__ __forceinline__ uint64_t wave_pick(uint64_t v, int src)
{
    return ((uint64_t)wave_pick((uint32_t)(v >> 32), src) << 32) | wave_pick((uint32_t)v, src);
}

constexpr int ASSIGN_BLOCK = 512;
constexpr uint32_t HIST_MAX = 8192;            // counters up to this: they gather in LDS first

// Window sources of assign_listed: begin(r) readies read r and returns its number of windows; owner_at(w) is the owner of window w's
// key (OWNER_SHARED when the window is not valid or its key is shared).

// nucleotide set: the read's k-windows, canonical keys
template <int KW>
struct NucWindows {
    const ReadsView &R; const KmerSetView &S; const uint32_t *__restrict__ owner; const int k;
    uint64_t b0 = 0; bool hasn = false;
    __device__ NucWindows(const ReadsView &R_, const KmerSetView &S_, const uint32_t *owner_) : R(R_), S(S_), owner(owner_), k(S_.k) {}
    __device__ __forceinline__ uint64_t begin(uint32_t r)
    {
        uint64_t len;
        if (R.uniform_len) { b0 = (uint64_t)r * R.uniform_len; len = R.uniform_len; }
        else { b0 = R.offsets[r]; len = R.offsets[r + 1] - b0; }
        hasn = (R.has_n[r >> 5] >> (r & 31)) & 1u;
        return len >= (uint64_t)k ? len - k + 1 : 0;
    }
    // no invalid base in window p
    __device__ __forceinline__ bool valid_at(uint64_t p) const
    {
        const uint64_t g = b0 + p;
        bool valid = true;
        if (hasn) { const uint64_t ni = npos_lower_bound(R, g); valid = !(ni < R.n_npos && R.npos[ni] < g + (uint64_t)k); }
        return valid;
    }
    __device__ __forceinline__ uint32_t owner_at(uint64_t p) const
    {
        uint32_t o = OWNER_SHARED;
        if (valid_at(p)) { const uint64_t slot = table_find(S, canonical_at<KW>(R.words, b0 + p, k)); if (slot != ~0ULL) o = owner[slot]; }
        return o;
    }
};

// The tally of one read over one sweep of its windows: a (key, count) map held one entry per lane in registers.  add() folds the 64
// lanes' keys into it with a ballot / readfirstlane leader loop, one distinct key per turn.  A read with more than 64 distinct keys is
// settled exactly by repeated sweeps: a full map keeps the 64 smallest keys it has seen (a key larger than all of them is skipped, the
// largest is evicted for a smaller newcomer), so after a sweep the map holds exact counts of the smallest keys, and the caller starts
// the next sweep behind them (next_bound()).  K: uint32_t or uint64_t; the all-ones key means none.
template <class K>
struct WaveTally {
    static constexpr K NONE = ~(K)0;
    K my_key = NONE; uint32_t my_cnt = 0;          // map entry `lane`
    uint32_t n_ent = 0; bool overflow = false;
    __device__ __forceinline__ void add(K id, int lane)
    {
        uint64_t pend = __ballot(id != NONE);
        while (pend) {                                                         // one distinct key a turn (wave-uniform)
            const K L = wave_pick(id, (int)(__ffsll((long long)pend) - 1));
            const uint64_t same = __ballot(id == L);
            const uint32_t c = (uint32_t)__popcll(same);
            pend &= ~same;
            const uint64_t hit = __ballot(my_key == L);
            if (hit) { if ((uint64_t)lane == (uint64_t)(__ffsll((long long)hit) - 1)) my_cnt += c; }
            else if (n_ent < 64) { if ((uint32_t)lane == n_ent) { my_key = L; my_cnt = c; } n_ent++; }
            else {                                                              // full: keep the 64 smallest keys
                overflow = true;
                const K mx = wave_max(my_key);
                if (L < mx) { if (my_key == mx) { my_key = L; my_cnt = c; } }
            }
        }
    }
    // this sweep's winner folded into the read's (best_cnt 0: none yet)
    __device__ __forceinline__ void fold(uint32_t &best_cnt, K &best_key, bool &tie) const
    {
        const uint32_t cmax = wave_max_u32(my_cnt);
        if (!cmax) return;
        const uint64_t at = __ballot(my_cnt == cmax);
        const K key = wave_pick(my_key, (int)(__ffsll((long long)at) - 1));
        if (cmax > best_cnt) { best_cnt = cmax; best_key = key; tie = __popcll(at) > 1; }
        else if (cmax == best_cnt) tie = true;
    }
    __device__ __forceinline__ K next_bound() const { return wave_max(my_key) + 1; }          // (a full map: every entry holds a key)
};

// Counters that many reads bump: most reads of a set go to a few of them, and same-address atomics serialise across the chip (one per
// read cost ~2 ms on 166 k passing reads): a wave's lane 0 adds runs of equal indices, a workgroup gathers them in LDS (when they fit
// HIST_MAX) and adds its non-zero entries at the end.  hist_begin / hist_end are called by the whole workgroup around the wave's work.
struct GatheredCounts {
    uint32_t *hist; unsigned long long *counts; uint32_t n; bool lds;
    uint32_t run_idx = 0, run_cnt = 0;             // (lane 0) the current run of equal indices
    __device__ GatheredCounts(uint32_t *s_hist, unsigned long long *counts_, uint32_t n_) : hist(s_hist), counts(counts_), n(n_), lds(n_ <= HIST_MAX) {}
    __device__ __forceinline__ void hist_begin()
    {
        if (lds) for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) hist[j] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void add(uint32_t idx, uint32_t c) { if (lds) atomicAdd(&hist[idx], c); else atomicAdd(&counts[idx], (unsigned long long)c); }
    __device__ __forceinline__ void bump(uint32_t idx)
    {
        if (run_cnt && idx == run_idx) run_cnt++;
        else { if (run_cnt) add(run_idx, run_cnt); run_idx = idx; run_cnt = 1; }
    }
    __device__ __forceinline__ void hist_end(int lane)
    {
        if (lane == 0 && run_cnt) add(run_idx, run_cnt);
        __syncthreads();
        if (lds) for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) if (hist[j]) atomicAdd(&counts[j], (unsigned long long)hist[j]);
    }
};

static inline unsigned grid_of(uint64_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

} // namespace mf
