// segsum.hip -- segmented row sum with the association pinned in segsum.h (chunks of EMD_SEG_CHUNK elements, fp64, ascending, one rounding).  gfx950.
// Two launches, both a pure function of the sorted keys: (1) one lane group per element; the groups that sit on a chunk start walk their chunk,
// (2) one lane group per possible chunk-0 of a run longer than a chunk; it adds that run's chunk sums.  No atomics, no fences.
#include "segsum.h"
#include "device_utils.h"

namespace {

#define EMD_SEGSUM_MAX_BLOCKS 16384          // launch 1: workgroups at most (its groups stride over the elements)

__device__ __forceinline__ uint32_t seg_n(const SegSumArgs& a) {
    const uint32_t cap = (uint32_t)a.n_cap, n = a.n_dev ? *a.n_dev : cap;
    return n < cap ? n : cap;            // (a count beyond the launch bound would index past the buffers)
}

// smallest s with keys[s] == key, given keys[hi] == key (keys non-decreasing)
__device__ __forceinline__ uint32_t run_first(const uint32_t* __restrict__ keys, uint32_t key, uint32_t hi) {
    uint32_t lo = 0;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// one past the last element with keys == key, given keys[at] == key
__device__ __forceinline__ uint32_t run_end(const uint32_t* __restrict__ keys, uint32_t key, uint32_t at, uint32_t n) {
    uint32_t lo = at + 1, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Launch 1.  Lane f of the group that visits element e owns float f of the rows.  The group's control flow is uniform: every ballot and shuffle below
// stays inside the group (other groups of the wave may have left or be in another trip).
template <int G>
__global__ void __launch_bounds__(EMD_BLOCK) k_segsum_chunks(SegSumArgs a) {
    const uint32_t n = seg_n(a);
    const uint32_t f = threadIdx.x % G, gbase = (threadIdx.x & 63u) & ~(uint32_t)(G - 1);
    const uint32_t* __restrict__ keys = a.keys;
    // the grid is bounded by the launch-time capacity but need not cover it: a group strides over the elements up to the device-side count
    // (4 x capacity slots against a few million contributions: as one group per slot the kernel spent its time on groups that only left)
    const size_t stride = (size_t)gridDim.x * (EMD_BLOCK / G);
    for (size_t gidx = ((size_t)blockIdx.x * EMD_BLOCK + threadIdx.x) / G; gidx < n; gidx += stride) {
        const uint32_t e = (uint32_t)gidx;
        const uint32_t key = keys[e];
        const bool head = e == 0 || keys[e - 1] != key;
        const bool deep = e >= EMD_SEG_CHUNK && keys[e - EMD_SEG_CHUNK] == key;       // a whole chunk of this run lies in front of e
        if (!head && !deep) continue;
        if (deep) {
            const uint32_t s = run_first(keys, key, e - EMD_SEG_CHUNK);
            if ((e - s) % EMD_SEG_CHUNK) continue;                                     // not a chunk start
        }
        const uint32_t lim = (n - e > EMD_SEG_CHUNK) ? e + EMD_SEG_CHUNK : n;
        double acc = 0.0;
        for (uint32_t base = e; base < lim; base += G) {
            // G elements at a time: keys and slots in one coalesced load, then the rows one after the other in element order
            const uint32_t j = base + f;
            const bool in = j < lim;
            const uint32_t kj = in ? keys[j] : 0u, sj = in ? a.slots[j] : 0u;
            const unsigned long long bits = (__ballot(in && kj == key) >> gbase) & ((1ull << G) - 1ull);
            const uint32_t m = (uint32_t)__builtin_ctzll(~bits);                       // leading elements of the batch that belong to the run (<= G)
            for (uint32_t t = 0; t < m; t++) {
                const uint32_t slot = (uint32_t)__shfl((int)sj, (int)t, G);
                if (f < (uint32_t)a.width) acc += (double)a.rows[(size_t)slot * a.row_pitch + f];
            }
            if (m < (uint32_t)G) break;
        }
        const bool lng = deep || (n - e > EMD_SEG_CHUNK && keys[e + EMD_SEG_CHUNK] == key);
        if (f < (uint32_t)a.width) {
            if (!lng) a.out[(size_t)key * a.out_pitch + f] = (float)acc;
            else {
                // a window of EMD_SEG_CHUNK elements holds at most two chunk starts of long runs: of the run that reaches into it (or starts with
                // it), and the first chunk of a run that starts inside it
                const uint32_t w = e / EMD_SEG_CHUNK;
                const size_t idx = 2 * (size_t)w + ((!deep && e > w * EMD_SEG_CHUNK) ? 1u : 0u);
                a.partials[idx * G + f] = acc;
            }
        }
    }
}

// Launch 2.  Group 2 w + k looks for the long run whose FIRST chunk owns partial slot 2 w + k and adds the run's chunk sums in chunk order.
template <int G>
__global__ void __launch_bounds__(EMD_BLOCK) k_segsum_long(SegSumArgs a) {
    const uint32_t n = seg_n(a);
    const size_t gidx = ((size_t)blockIdx.x * EMD_BLOCK + threadIdx.x) / G;
    const size_t w0 = (gidx >> 1) * EMD_SEG_CHUNK;
    if (w0 >= n) return;
    const uint32_t f = threadIdx.x % G;
    const uint32_t* __restrict__ keys = a.keys;
    uint32_t s, key;
    if (!(gidx & 1)) {                           // a run that starts with the window
        s = (uint32_t)w0; key = keys[s];
        if (s > 0 && keys[s - 1] == key) return;
    } else {                                     // a run that starts inside it: being long, it holds the window's last element and the one behind
        const size_t last = w0 + EMD_SEG_CHUNK - 1;
        if (last + 1 >= n) return;
        key = keys[last];
        if (keys[last + 1] != key) return;
        s = run_first(keys, key, (uint32_t)last);
        if (s <= w0) return;
    }
    if (n - s <= EMD_SEG_CHUNK || keys[s + EMD_SEG_CHUNK] != key) return;          // one chunk: written by launch 1
    const uint32_t end = run_end(keys, key, s + EMD_SEG_CHUNK, n);
    const uint32_t nch = (end - s + EMD_SEG_CHUNK - 1) / EMD_SEG_CHUNK;
    if (f >= (uint32_t)a.width) return;
    double tot = 0.0;
    for (uint32_t c = 0; c < nch; c++) {
        const size_t idx = c == 0 ? gidx : 2 * (size_t)((s + c * EMD_SEG_CHUNK) / EMD_SEG_CHUNK);
        tot += a.partials[idx * G + f];
    }
    a.out[(size_t)key * a.out_pitch + f] = (float)tot;
}

template <int G>
int launch(const SegSumArgs& a, hipStream_t st) {
    const size_t groups1 = a.n_cap, groups2 = 2 * ((a.n_cap + EMD_SEG_CHUNK - 1) / EMD_SEG_CHUNK), per = EMD_BLOCK / G;
    const size_t blocks1 = (groups1 + per - 1) / per;
    hipLaunchKernelGGL(k_segsum_chunks<G>, dim3((unsigned)(blocks1 < EMD_SEGSUM_MAX_BLOCKS ? blocks1 : EMD_SEGSUM_MAX_BLOCKS)), dim3(EMD_BLOCK), 0, st, a);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_segsum_long<G>, dim3((unsigned)((groups2 + per - 1) / per)), dim3(EMD_BLOCK), 0, st, a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

}  // namespace

int emd_launch_segmented_row_sum(const SegSumArgs& a, hipStream_t st) {
    if (a.n_cap == 0) return EMD_OK;
    return emd_segsum_group(a.width) == 16 ? launch<16>(a, st) : launch<32>(a, st);
}

extern "C" size_t emd_segmented_row_sum_workspace(int64_t n_cap, int32_t width) {
    if (n_cap < 0 || width < 1 || width > 32) return 0;
    return emd_segsum_partial_bytes((size_t)n_cap, width);
}

// The sum on its own (include/emd_raster.h): validates, then marshals the C struct into SegSumArgs; nothing is launched for a bad argument.
extern "C" int emd_segmented_row_sum(const EmdSegSumArgs* a, void* hip_stream) {
    if (!a) { emd_set_error("segmented_row_sum: null args"); return EMD_ERR_INVALID; }
    if (a->n_cap < 0 || a->n_cap > (int64_t)0xFFFFFFFFu - EMD_SORT_TILE) { emd_set_error("segmented_row_sum: n_cap %lld is negative or too large for 32-bit positions", (long long)a->n_cap); return EMD_ERR_INVALID; }
    if (a->width < 1 || a->width > 32 || a->row_pitch < a->width || a->out_pitch < a->width) {
        emd_set_error("segmented_row_sum: need 1 <= width <= 32 and width <= row_pitch, out_pitch (width %d, pitches %d / %d)", a->width, a->row_pitch, a->out_pitch);
        return EMD_ERR_INVALID;
    }
    if (a->n_cap > 0 && (!a->keys || !a->slots || !a->rows || !a->out || !a->partials)) { emd_set_error("segmented_row_sum: null keys / slots / rows / out / partials pointer"); return EMD_ERR_INVALID; }
    if ((uintptr_t)a->partials & 7) { emd_set_error("segmented_row_sum: partials must be 8-byte aligned"); return EMD_ERR_INVALID; }
    if (a->partial_bytes < emd_segsum_partial_bytes((size_t)a->n_cap, a->width)) {
        emd_set_error("segmented_row_sum: partials hold %zu bytes, %zu needed", a->partial_bytes, emd_segsum_partial_bytes((size_t)a->n_cap, a->width));
        return EMD_ERR_WORKSPACE;
    }
    SegSumArgs s;
    s.keys = a->keys; s.slots = a->slots; s.n_dev = a->n_dev; s.n_cap = (size_t)a->n_cap;
    s.rows = a->rows; s.row_pitch = a->row_pitch; s.width = a->width;
    s.out = a->out; s.out_pitch = a->out_pitch; s.partials = a->partials;
    return emd_launch_segmented_row_sum(s, (hipStream_t)hip_stream);
}
