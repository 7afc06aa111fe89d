// fixed_sum.h -- sums of doubles whose association is fixed by the source, for the units whose outputs are a fixed function of their inputs
// (plane_reg.hip, vanilla.hip, trainer_loss.hip): the lanes of a wave in one xor tree, the four waves of a workgroup as (0 + 1) + (2 + 3).  No atomics.
// The finalize kernels of those units add the workgroups' partials with column associations of their own, which are part of each contract's bits.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ double fixed_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);          // a fixed tree; every lane ends with the same bits
    return v;
}

// N per-lane doubles -> the workgroup's sums at out[0 .. N): lanes in a fixed tree, the four waves left to right
template <int N>
__device__ __forceinline__ void fixed_block_store(const double (&v)[N], double* __restrict__ out) {
    __shared__ double sm[EMD_BLOCK / EMD_WAVE][N];
#pragma unroll
    for (int q = 0; q < N; q++) {
        const double s = fixed_wave_sum(v[q]);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) out[threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

}  // namespace
