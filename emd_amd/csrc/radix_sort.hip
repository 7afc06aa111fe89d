// radix_sort.hip -- stable LSD radix sort of (32-bit key, 32-bit value) pairs: the interface is radix_sort.h.
// A pass is three launches on the caller's capacity: (a) digit histogram of every block of 2048 keys, (b) scan over [bin][block], one workgroup per
// digit, (c) stable scatter.  Ranking inside a block is wave-ballot based (BITS ballots per key give the set of lanes with the same digit; no LDS
// atomics in the ranking loop), which keeps every pass stable.  The element count may live on the device (SortN), so a sort needs no host read-back.
#include "radix_sort.h"
#include "device_utils.h"

namespace {

// number of elements of a radix pass: a launch-time constant (first pass of the Gaussian depth sort), or a device-side count
// (visible Gaussians after that pass; the duplicate count of the tile passes) that reads as 0 while the overflow word is set
struct SortN { const uint32_t* count; const uint32_t* overflow; uint32_t fixed; };
__device__ __forceinline__ uint32_t sort_n(const SortN& c) {
    return c.count ? ((c.overflow && *c.overflow) ? 0u : *c.count) : c.fixed;
}

// ---------------------------------------------------------------------------------------------------
// scan geometry of the single-workgroup scans below: 1024 elements per trip
// ---------------------------------------------------------------------------------------------------
#define SCAN_ITEMS 4
#define SCAN_TILE (EMD_BLOCK * SCAN_ITEMS)

// ---------------------------------------------------------------------------------------------------
// K4 radix pass on 32-bit keys with 32-bit values: (a) block histograms, (b) scan over [bin][block], (c) stable scatter.
// BITS = 8 (256 digits: the tile passes, the wide depth sort) or 9 (512 digits: the usual three-pass depth sort).
// `offset` is subtracted from every key before the digit is taken (depth bits relative to the near plane's).
// FIRST (first pass of the depth sort): the value of element idx is idx itself, culled Gaussians (key 0xFFFFFFFF) are skipped --
// they take part in neither the counts nor the scatter, so this stable pass also compacts the N Gaussians to the V visible
// ones in index order, and block 0 publishes V for the later passes; keys that do not fit `range_bits` raise bit 1 of the
// overflow word (the host then switches that camera to the wide sort, like a capacity overflow).
// ---------------------------------------------------------------------------------------------------
template <int BITS, bool FIRST>
__global__ void __launch_bounds__(EMD_BLOCK) k_radix_hist(const uint32_t* __restrict__ keys, SortN cnt, int shift, uint32_t mask, uint32_t offset,
                                                          uint32_t nblocks_cap, uint32_t* __restrict__ hist, int range_bits,
                                                          uint32_t* __restrict__ overflow_word) {
    constexpr int BINS = 1 << BITS, PER = BINS / EMD_BLOCK;
    __shared__ uint32_t s_h[BINS];
    const uint32_t D = sort_n(cnt);
    const uint32_t nblocks = (D + EMD_SORT_TILE - 1) / EMD_SORT_TILE;
#pragma unroll
    for (int k = 0; k < PER; k++) s_h[threadIdx.x + k * EMD_BLOCK] = 0;
    __syncthreads();
    if (blockIdx.x < nblocks) {
        const size_t base = (size_t)blockIdx.x * EMD_SORT_TILE;
        bool wide = false;
        // all of the thread's keys first, unconditionally (an index past the end reads the last key and is not counted): with the load inside the
        // guard the compiler waited for every key before asking for the next -- eight trips to memory one after the other per workgroup
        uint32_t kv[EMD_SORT_ITEMS];
#pragma unroll
        for (int k = 0; k < EMD_SORT_ITEMS; k++) {
            const size_t idx = base + (size_t)k * EMD_BLOCK + threadIdx.x;
            kv[k] = keys[idx < D ? idx : (size_t)D - 1];
        }
#pragma unroll
        for (int k = 0; k < EMD_SORT_ITEMS; k++) {
            size_t idx = base + (size_t)k * EMD_BLOCK + threadIdx.x;
            if (idx < D) {
                const uint32_t key = kv[k];
                if (FIRST && key == 0xFFFFFFFFu) continue;
                const uint32_t rel = key - offset;
                if (FIRST && range_bits < 32 && (rel >> range_bits)) wide = true;
                atomicAdd(&s_h[(rel >> shift) & mask], 1u);
            }
        }
        if (FIRST && wide) atomicOr(overflow_word, 2u);
    }
    __syncthreads();
    // bin-major layout over the *capacity* block count so the scan length is launch-time constant
#pragma unroll
    for (int k = 0; k < PER; k++) hist[(size_t)(threadIdx.x + k * EMD_BLOCK) * nblocks_cap + blockIdx.x] = s_h[threadIdx.x + k * EMD_BLOCK];
}

// One workgroup per digit: inclusive scan of that digit's per-block counts (row `bin` of the bin-major table) in place.
// Replaces three launch-bound generic scan launches per pass; the cross-digit offsets are formed in the scatter kernel.
__global__ void __launch_bounds__(EMD_BLOCK) k_radix_scan_bins(uint32_t* __restrict__ hist, uint32_t nblocks_cap) {
    __shared__ uint32_t s[4];
    uint32_t* row = hist + (size_t)blockIdx.x * nblocks_cap;
    uint32_t carry = 0;
    // the counts of the NEXT tile travel while this one is scanned (two barriers and the stores): unconditional loads from clamped positions, masked
    // where they are used -- a row of a few thousand counts was load -> scan -> store, one round trip per 1024 counts in a 5 us kernel
    uint32_t nv[SCAN_ITEMS];
    const uint32_t last = nblocks_cap ? nblocks_cap - 1 : 0u;
    auto request = [&](uint32_t base) {
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) nv[k] = row[min(base + threadIdx.x * SCAN_ITEMS + k, last)];
    };
    request(0);
    for (uint32_t base = 0; base < nblocks_cap; base += SCAN_TILE) {
        const uint32_t i0 = base + threadIdx.x * SCAN_ITEMS;
        uint32_t v[SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) { v[k] = (i0 + k < nblocks_cap) ? nv[k] : 0u; sum += v[k]; }
        request(base + SCAN_TILE);                    // (past the end: the row's last count again, unused)
        uint32_t total;
        const uint32_t inc = block_scan_add_u32(sum, s, &total);
        uint32_t run = carry + inc - sum;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; k++) { run += v[k]; if (i0 + k < nblocks_cap) row[i0 + k] = run; }
        carry += total;
    }
}

template <int BITS, bool FIRST>
__global__ void __launch_bounds__(EMD_BLOCK) k_radix_scatter(const uint32_t* __restrict__ keys_in,
                                                             const uint32_t* __restrict__ vals_in,
                                                             uint32_t* __restrict__ keys_out,
                                                             uint32_t* __restrict__ vals_out, SortN cnt, int shift,
                                                             uint32_t mask, uint32_t offset, uint32_t nblocks_cap,
                                                             const uint32_t* __restrict__ hist_inc, uint32_t* __restrict__ count_out) {
    // wave w of the block owns the contiguous slice [w*512, (w+1)*512) of the block's 2048 keys and walks it in
    // 8 rounds of 64 consecutive keys: order inside the block = (wave, round, lane) = memory order => stable.
    constexpr int BINS = 1 << BITS, PER = BINS / EMD_BLOCK;
    __shared__ uint32_t s_cnt[4][BINS];   // running per-wave digit counts, then per-wave bases
    __shared__ uint32_t s_gbase[BINS];
    __shared__ uint32_t s_keys[EMD_SORT_TILE];
    __shared__ uint32_t s_vals[EMD_SORT_TILE];
    __shared__ uint32_t s_scan[4];
    const uint32_t D = sort_n(cnt);
    const uint32_t nblocks = (D + EMD_SORT_TILE - 1) / EMD_SORT_TILE;
    if (blockIdx.x >= nblocks) {
        // an empty input (a device-side count of 0, or one voided by its overflow word) still publishes its count: the later passes read it
        if (FIRST && count_out && blockIdx.x == 0 && threadIdx.x == 0) *count_out = 0u;
        return;
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < PER; j++) s_cnt[k][threadIdx.x + j * EMD_BLOCK] = 0;
    __syncthreads();
    const size_t wbase = (size_t)blockIdx.x * EMD_SORT_TILE + (size_t)wave * (EMD_SORT_TILE / 4);
    uint32_t key[EMD_SORT_ITEMS];
    uint32_t val[EMD_SORT_ITEMS];
    uint32_t rank[EMD_SORT_ITEMS];
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    // all loads of the block first (keys, values, the digit rows of the scanned histogram further down): one round trip, not three
#pragma unroll
    for (int k = 0; k < EMD_SORT_ITEMS; k++) {
        const size_t idx = wbase + (size_t)k * 64 + lane;
        key[k] = idx < D ? keys_in[idx] : 0xFFFFFFFFu;
        val[k] = FIRST ? (uint32_t)idx : (idx < D ? vals_in[idx] : 0u);
    }
    uint32_t h_before[PER], h_tot[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const uint32_t* row = hist_inc + (size_t)(threadIdx.x * PER + j) * nblocks_cap;       // a thread owns PER consecutive digits
        h_before[j] = blockIdx.x ? row[blockIdx.x - 1] : 0u;
        h_tot[j] = row[nblocks_cap - 1];
    }
#pragma unroll
    for (int k = 0; k < EMD_SORT_ITEMS; k++) {
        const size_t idx = wbase + (size_t)k * 64 + lane;
        bool valid = idx < D;
        if (FIRST) valid = valid && key[k] != 0xFFFFFFFFu;          // culled Gaussian: dropped here
        const uint32_t digit = ((key[k] - offset) >> shift) & mask;
        // lanes with the same digit (invalid lanes form their own class and are ignored)
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            const unsigned long long bal = __ballot((digit >> b) & 1u);
            same &= ((digit >> b) & 1u) ? bal : ~bal;
        }
        const uint32_t before = (uint32_t)__popcll(same & lt_mask);
        const uint32_t prev = s_cnt[wave][digit];          // count from earlier rounds of this wave
        rank[k] = valid ? prev + before : 0xFFFFFFFFu;
        // the highest lane of each class publishes the new count (wave-private row: no atomics, no race)
        const bool leader = valid && ((same >> lane) >> 1) == 0ull;
        __builtin_amdgcn_wave_barrier();
        if (leader) s_cnt[wave][digit] = prev + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // per-wave bases in the block's digit-sorted order + the block's global base for every digit
    {
        uint32_t c[PER][4], csum[PER], dtot[PER], before[PER];
        uint32_t csum_t = 0, dtot_t = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const uint32_t d = threadIdx.x * PER + j;       // a thread owns PER consecutive digits
#pragma unroll
            for (int w = 0; w < 4; w++) c[j][w] = s_cnt[w][d];
            csum[j] = c[j][0] + c[j][1] + c[j][2] + c[j][3];
            // keys of digit d in earlier blocks (row-wise inclusive scan) + all keys of smaller digits (row totals)
            before[j] = h_before[j];
            dtot[j] = h_tot[j];
            csum_t += csum[j]; dtot_t += dtot[j];
        }
        uint32_t total;
        uint32_t g = block_scan_add_u32(dtot_t, s_scan, &total) - dtot_t;
        if (FIRST && count_out && blockIdx.x == 0 && threadIdx.x == 0) *count_out = total;      // V: elements of the later passes
        uint32_t bpre = block_scan_add_u32(csum_t, s_scan, &total) - csum_t;
        __syncthreads();                                    // every thread has read its s_cnt columns
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const uint32_t d = threadIdx.x * PER + j;
            s_gbase[d] = g + before[j] - bpre;              // global slot = s_gbase[digit] + position in block order
            s_cnt[0][d] = bpre;
            s_cnt[1][d] = bpre + c[j][0];
            s_cnt[2][d] = bpre + c[j][0] + c[j][1];
            s_cnt[3][d] = bpre + c[j][0] + c[j][1] + c[j][2];
            g += dtot[j]; bpre += csum[j];
        }
    }
    __syncthreads();
    // Reorder inside LDS first, then write: consecutive lanes hold consecutive output slots, so every digit run
    // leaves the block as one contiguous segment.  Scattering straight from registers wrote 4-byte fragments
    // of 256 different runs: 2.2x write amplification at the memory side (profiles/r01_pmc_hbm_traffic.csv).
    uint32_t nvalid_w = 0;
#pragma unroll
    for (int k = 0; k < EMD_SORT_ITEMS; k++) {
        if (rank[k] != 0xFFFFFFFFu) {
            const uint32_t digit = ((key[k] - offset) >> shift) & mask;
            const uint32_t pos = s_cnt[wave][digit] + rank[k];
            s_keys[pos] = key[k];
            s_vals[pos] = val[k];
            nvalid_w++;
        }
    }
    uint32_t nvalid;
    block_scan_add_u32(nvalid_w, s_scan, &nvalid);         // (ends with a barrier: the reordered tile is complete)
#pragma unroll
    for (int k = 0; k < EMD_SORT_ITEMS; k++) {
        const uint32_t pos = threadIdx.x + (uint32_t)k * EMD_BLOCK;
        if (pos < nvalid) {
            const uint32_t kk = s_keys[pos];
            const size_t dst = (size_t)s_gbase[((kk - offset) >> shift) & mask] + pos;
            keys_out[dst] = kk;
            vals_out[dst] = s_vals[pos];
        }
    }
}

// pass p of the sort: histogram (unless the producer built it), digit scan, scatter.  FIRST: pass 0 of a compacting sort
template <int BITS, bool FIRST>
int radix_pass(const RadixSortArgs& a, int p, hipStream_t st) {
    const bool compacting = a.keys_in != nullptr;
    const int in = emd_radix_result_buf(compacting, p), out = emd_radix_result_buf(compacting, p + 1), shift = p * a.bits;
    const uint32_t *kin = FIRST ? a.keys_in : a.keys[in], *vin = FIRST ? nullptr : a.vals[in];
    const SortN cnt = (compacting && !FIRST) ? SortN{a.count_out, nullptr, 0u} : SortN{a.n_dev, a.n_dev_overflow, a.n_dev ? 0u : (uint32_t)a.n_cap};
    const uint32_t nsb = (uint32_t)((a.n_cap + EMD_SORT_TILE - 1) / EMD_SORT_TILE), mask = (1u << a.bits) - 1u;
    if (!(p == 0 && a.hist0_ready)) {
        hipLaunchKernelGGL((k_radix_hist<BITS, FIRST>), dim3(nsb), dim3(EMD_BLOCK), 0, st, kin, cnt, shift, mask, a.offset, nsb, a.hist,
                           FIRST ? a.range_bits : 32, a.overflow_word);
        EMD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_radix_scan_bins, dim3(1u << BITS), dim3(EMD_BLOCK), 0, st, a.hist, nsb);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_radix_scatter<BITS, FIRST>), dim3(nsb), dim3(EMD_BLOCK), 0, st, kin, vin, a.keys[out], a.vals[out], cnt, shift, mask, a.offset, nsb,
                       a.hist, FIRST ? a.count_out : (uint32_t*)nullptr);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

}  // namespace

int emd_launch_radix_sort(const RadixSortArgs& a, hipStream_t st) {
    const bool compacting = a.keys_in != nullptr;
    for (int p = 0; p < a.passes && a.n_cap; p++) {
        const bool first = compacting && p == 0;
        const int rc = a.bits == 9 ? (first ? radix_pass<9, true>(a, p, st) : radix_pass<9, false>(a, p, st))
                                   : (first ? radix_pass<8, true>(a, p, st) : radix_pass<8, false>(a, p, st));
        if (rc) return rc;
    }
    return emd_radix_result_buf(compacting, a.passes);
}

// The sort on its own (include/emd_raster.h): marshals the C struct into RadixSortArgs after validating it; nothing is launched for a bad argument.
extern "C" int emd_radix_sort(const EmdRadixSortArgs* a, void* hip_stream) {
    if (!a) { emd_set_error("radix_sort: null args"); return EMD_ERR_INVALID; }
    if (!a->keys[0] || !a->keys[1] || !a->vals[0] || !a->vals[1] || !a->hist) { emd_set_error("radix_sort: null keys / vals / hist pointer"); return EMD_ERR_INVALID; }
    if (a->bits < 1 || a->bits > 9) { emd_set_error("radix_sort: bits %d outside 1..9", a->bits); return EMD_ERR_INVALID; }
    if (a->passes < 0 || (int64_t)a->passes * a->bits > 32) { emd_set_error("radix_sort: passes %d: need passes >= 0 and passes * bits <= 32", a->passes); return EMD_ERR_INVALID; }
    const bool compacting = a->keys_in != nullptr;
    if (compacting && (a->passes < 1 || !a->count_out)) { emd_set_error("radix_sort: a compacting sort needs passes >= 1 and count_out"); return EMD_ERR_INVALID; }
    if (a->range_bits < 0 || a->range_bits > 32) { emd_set_error("radix_sort: range_bits %d outside 0..32", a->range_bits); return EMD_ERR_INVALID; }
    if (a->range_bits < 32 && !a->overflow_word) { emd_set_error("radix_sort: range_bits < 32 needs overflow_word"); return EMD_ERR_INVALID; }
    if (a->n_dev_overflow && !a->n_dev) { emd_set_error("radix_sort: n_dev_overflow without n_dev"); return EMD_ERR_INVALID; }
    // positions and counts are 32-bit on the device, rounded up to whole blocks of EMD_SORT_TILE keys
    if (a->n_cap < 0 || a->n_cap > (int64_t)0xFFFFFFFFu - EMD_SORT_TILE) { emd_set_error("radix_sort: n_cap %lld is negative or too large for 32-bit positions", (long long)a->n_cap); return EMD_ERR_INVALID; }
    RadixSortArgs r;
    r.keys_in = a->keys_in;
    for (int i = 0; i < 2; i++) { r.keys[i] = a->keys[i]; r.vals[i] = a->vals[i]; }
    r.hist = a->hist;
    r.n_cap = (size_t)a->n_cap;
    r.n_dev = a->n_dev;
    r.n_dev_overflow = a->n_dev_overflow;
    r.passes = a->passes;
    r.bits = a->bits;
    r.offset = a->offset;
    r.range_bits = a->range_bits;
    r.overflow_word = a->overflow_word;
    r.count_out = a->count_out;
    return emd_launch_radix_sort(r, (hipStream_t)hip_stream);          // (n_cap == 0: no launch, the result index alone)
}
