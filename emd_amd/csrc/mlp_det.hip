// mlp_det.hip -- the deterministic forms of the MLP kernels of mlp.hip: no float atomics.
//
// The default kernels run as persistent workgroups (mlp_grid: a function of num_points alone), a wave walks its tiles in ascending order, the four
// waves of a workgroup are added through LDS in a fixed order -- and only then one float atomic per element and workgroup reaches HBM: the order in
// which the up to 512 workgroups hit an address is the one scheduling-dependent step.  The kernels here are the SAME bodies (mlp_*_body.inc) with the
// other flush policy: wave 0 stores the workgroup's total to slot blockIdx.x of a slab [G][pitch] per gradient tensor, with the bounds of the atomic
// flush, so every workgroup writes every element of its slot and the slab is never cleared.  k_mlp_det_reduce then adds the G slots of every
// destination element in ascending order in double precision from 0.0, scales, rounds once and writes -- one launch for every tensor of a level and
// direction (a table of jobs passed by value).  The head forward's sum |out| (EmdMlpBranch.l1_sum) takes the same road through a [G] slab.
// Only the backward forms and the L1 forward forms exist here; the dispatch and the refusals are the default entry points' own functions.
#include "mlp_kernels.h"

namespace {

template <int DEPTH, int NTO, bool L1, bool RC>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(branch_fwd_waves(DEPTH, NTO)) k_mlp_branch_fwd_det(EmdMlpBranch a, DetSlabs slabs) {
    const FlushSlab fl{slabs};
#include "mlp_branch_fwd_body.inc"
}

template <int DEPTH, int NTO, bool L1, bool RC, int GO, bool CHAIN>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(branch_bwd_waves) k_mlp_branch_bwd_det(EmdMlpBranch a, EmdMlpBranchGrads g, DetSlabs slabs) {
    const FlushSlab fl{slabs};
#include "mlp_branch_bwd_body.inc"
}

template <int KTA, bool MULTI>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(trunk_bwd_waves(KTA)) k_mlp_trunk_bwd_det(EmdMlpTrunk a, EmdMlpTrunkGrads g, DetSlabs slabs) {
    const FlushSlab fl{slabs};
#include "mlp_trunk_bwd_body.inc"
}

template <int KB, bool MULTI>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(embed_bwd_waves) k_mlp_embed_bwd_det(EmdMlpTrunk a, EmdMlpTrunkGrads g, DetSlabs slabs) {
    const FlushSlab fl{slabs};
#include "mlp_embed_bwd_body.inc"
}

struct Kernels {
    template <int DEPTH, int NTO, bool L1, bool RC> static constexpr auto branch_fwd = &k_mlp_branch_fwd_det<DEPTH, NTO, L1, RC>;
    template <int DEPTH, int NTO, bool L1, bool RC, int GO, bool CHAIN> static constexpr auto branch_bwd = &k_mlp_branch_bwd_det<DEPTH, NTO, L1, RC, GO, CHAIN>;
    template <int KTA, bool MULTI> static constexpr auto trunk_bwd = &k_mlp_trunk_bwd_det<KTA, MULTI>;
    template <int KB, bool MULTI> static constexpr auto embed_bwd = &k_mlp_embed_bwd_det<KB, MULTI>;
};

// ---- the reduction: element e = o cols + i of job blockIdx.y <- (float)(scale * sum_{slot ascending} slab[slot][e]), in double precision from 0.0
#define DET_REDUCE_THREADS 256
struct DetJobs { EmdMlpDetJob job[EMD_MLP_DET_MAX_JOBS]; };
__global__ void __launch_bounds__(DET_REDUCE_THREADS) k_mlp_det_reduce(DetJobs jobs) {
    const EmdMlpDetJob& j = jobs.job[blockIdx.y];
    const int total = j.rows * j.cols;
    for (int e = blockIdx.x * DET_REDUCE_THREADS + threadIdx.x; e < total; e += gridDim.x * DET_REDUCE_THREADS) {
        const float* __restrict__ p = j.slab + e;
        double acc = 0.0;
        for (int s = 0; s < j.groups; s++) acc += (double)p[(size_t)s * j.pitch];
        const int o = e / j.cols, i = e - o * j.cols;
        j.dst[(size_t)o * j.ld + j.col0 + i] = (float)(acc * j.scale);
    }
}

size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the slab of a call: G from the grid of the kernel that serves it, the pitches from the shapes.  Returns false for a call the entry points refuse.
bool det_layout(int kind, const void* args, const void* grads, EmdMlpDetLayout* out) {
    EmdMlpDetLayout L;
    memset(&L, 0, sizeof(L));
    int n = 0, per_cu = 1;
    if (kind == EMD_MLP_DET_BRANCH_BWD || kind == EMD_MLP_DET_BRANCH_FWD) {
        const EmdMlpBranch* a = (const EmdMlpBranch*)args;
        if (!a || a->num_points < 0 || (a->depth != 1 && a->depth != 2) || a->out_dim < 1 || a->out_dim > 64) return false;
        n = a->num_points;
        if (kind == EMD_MLP_DET_BRANCH_FWD) {
            per_cu = branch_forward_per_cu(a);
            L.num_tensors = 1;
            L.pitch[0] = 1;
        } else {
            per_cu = branch_bwd_waves;
            L.num_tensors = 6;
            L.pitch[0] = 64 * 64; L.pitch[1] = 64;
            if (a->depth == 2) { L.pitch[2] = 64 * 64; L.pitch[3] = 64; }
            L.pitch[4] = 64 * a->out_dim; L.pitch[5] = a->out_dim;
        }
    } else if (kind == EMD_MLP_DET_TRUNK_BWD) {
        const EmdMlpTrunk* a = (const EmdMlpTrunk*)args;
        if (!a || a->num_points < 0 || a->ka < 0 || a->ka > 128 || (a->ka & 3) || a->kb < 0 || a->kb > 8 || a->ka + a->kb == 0) return false;
        n = a->num_points;
        EmdMlpTrunkGrads none;
        memset(&none, 0, sizeof(none));
        per_cu = trunk_backward_per_cu(a, grads ? (const EmdMlpTrunkGrads*)grads : &none);
        L.num_tensors = 3;
        L.pitch[0] = 64 * a->ka; L.pitch[1] = 64 * a->kb; L.pitch[2] = 64;
    } else return false;
    if (n > 0) {
        L.groups = (int32_t)mlp_grid(n, per_cu);
        size_t off = 0;
        for (int t = 0; t < L.num_tensors; t++) {
            L.offset[t] = off;
            off += round256((size_t)L.groups * L.pitch[t] * sizeof(float));
        }
        L.bytes = off;
    }
    *out = L;
    return true;
}

// the slab pointers of a call, or EMD_ERR_WORKSPACE: decided before anything is launched
int det_slabs(int kind, const void* args, const void* grads, void* slab, size_t slab_bytes, const char* who, DetSlabs* s) {
    EmdMlpDetLayout L;
    if (!det_layout(kind, args, grads, &L)) { emd_set_error("%s: bad sizes", who); return EMD_ERR_INVALID; }
    if (!slab || ((uintptr_t)slab & 255) || slab_bytes < L.bytes) {
        emd_set_error("%s: the slab is missing, not 256-byte aligned or shorter than emd_mlp_det_slab_bytes reports (%zu < %zu)", who, slab_bytes, L.bytes);
        return EMD_ERR_WORKSPACE;
    }
    for (int t = 0; t < EMD_MLP_DET_MAX_TENSORS; t++) s->p[t] = (float*)((char*)slab + L.offset[t]);
    return EMD_OK;
}

}  // namespace

extern "C" size_t emd_mlp_det_slab_bytes(int kind, const void* args, const void* grads, EmdMlpDetLayout* layout) {
    EmdMlpDetLayout L;
    if (!det_layout(kind, args, grads, &L)) return 0;
    if (layout) *layout = L;
    return L.bytes;
}

extern "C" int emd_mlp_branch_forward_det(const EmdMlpBranch* a, void* l1_slab, size_t slab_bytes, void* hip_stream) {
    int rc = check_branch_forward(a, "mlp_branch_forward_det");
    if (rc || a->num_points == 0) return rc;
    if (!a->l1_sum) { emd_set_error("mlp_branch_forward_det: l1_sum is what this form is for (emd_mlp_branch_forward has no atomics without it)"); return EMD_ERR_INVALID; }
    DetSlabs s;
    rc = det_slabs(EMD_MLP_DET_BRANCH_FWD, a, nullptr, l1_slab, slab_bytes, "mlp_branch_forward_det", &s);
    if (rc) return rc;
    return branch_forward_dispatch<Kernels, true>(a, (hipStream_t)hip_stream, s);
}

extern "C" int emd_mlp_branch_backward_det(const EmdMlpBranch* a, const EmdMlpBranchGrads* g, void* slabs, size_t slab_bytes, void* hip_stream) {
    int rc = check_branch_backward(a, g, "mlp_branch_backward_det");
    if (rc || a->num_points == 0) return rc;
    DetSlabs s;
    rc = det_slabs(EMD_MLP_DET_BRANCH_BWD, a, g, slabs, slab_bytes, "mlp_branch_backward_det", &s);
    if (rc) return rc;
    return branch_backward_dispatch<Kernels>(a, g, (hipStream_t)hip_stream, s);
}

extern "C" int emd_mlp_trunk_backward_det(const EmdMlpTrunk* a, const EmdMlpTrunkGrads* g, void* slabs, size_t slab_bytes, void* hip_stream) {
    int rc = check_trunk_backward(a, g, "mlp_trunk_backward_det");
    if (rc || a->num_points == 0) return rc;
    DetSlabs s;
    rc = det_slabs(EMD_MLP_DET_TRUNK_BWD, a, g, slabs, slab_bytes, "mlp_trunk_backward_det", &s);
    if (rc) return rc;
    return trunk_backward_dispatch<Kernels>(a, g, (hipStream_t)hip_stream, s);
}

extern "C" int emd_mlp_det_reduce(const EmdMlpDetJob* jobs, int num_jobs, void* hip_stream) {
    if (!jobs || num_jobs < 1 || num_jobs > EMD_MLP_DET_MAX_JOBS) { emd_set_error("mlp_det_reduce: 1..%d jobs", EMD_MLP_DET_MAX_JOBS); return EMD_ERR_INVALID; }
    DetJobs table;
    memset(&table, 0, sizeof(table));
    int most = 0;
    for (int k = 0; k < num_jobs; k++) {
        const EmdMlpDetJob& j = jobs[k];
        if (!j.slab || !j.dst || j.groups < 1 || j.rows < 1 || j.cols < 1 || (int64_t)j.rows * j.cols > (int64_t)j.pitch || j.col0 < 0 || j.ld < j.col0 + j.cols) {
            emd_set_error("mlp_det_reduce: job %d: null pointer or bad sizes", k); return EMD_ERR_INVALID;
        }
        table.job[k] = j;
        most = j.rows * j.cols > most ? j.rows * j.cols : most;
    }
    hipLaunchKernelGGL(k_mlp_det_reduce, dim3((most + DET_REDUCE_THREADS - 1) / DET_REDUCE_THREADS, num_jobs), dim3(DET_REDUCE_THREADS), 0, (hipStream_t)hip_stream, table);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
