/*
 * emd_raster.h -- C ABI of the MI355X (gfx950) street-Gaussian rasterizer.
 *
 * This is the drop-in boundary for EMD's hot path.  The reference binds this path
 * through a third-party CUDA extension that is NOT vendored in the reference tree
 * (`from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer`,
 * S3Gaussian/gaussian_renderer/__init__.py:14; `gsplat.rendering.rasterization`,
 * OmniRe/models/gaussians/basics.py:12).  The entry points below are what a Python
 * `ctypes` binding of that path binds instead:
 *
 *   emd_raster_forward   <- GaussianRasterizer.forward(...)   S3Gaussian/gaussian_renderer/__init__.py:145-155
 *                           rasterization(...)                OmniRe/models/trainers/base.py:393-408
 *   emd_raster_backward  <- autograd of the same call         S3Gaussian/train.py:366
 *   emd_motion_forward / emd_motion_backward / emd_motion_backward_det
 *                        <- RigidNodes.transform_means/quats  OmniRe/models/nodes/rigid.py:478-568
 *                           DeformableNodes residual add      OmniRe/models/nodes/deformable.py:57-69
 *                           (when EMD_FLAG_MOTION is set the same transform is fused
 *                            into the projection kernel of emd_raster_forward)
 *   emd_sh_forward / emd_sh_backward
 *                        <- gsplat spherical_harmonics(...)   OmniRe/models/nodes/rigid.py:584
 *
 * and, further down, the callers either side of that path, each with its own block comment:
 *   emd_sky_forward / backward          <- SkyCubeMap.forward + blend    S3Gaussian/scene/sky_cubemap.py:41-87, gaussian_renderer/__init__.py:299-301
 *                                          EnvLight.forward              OmniRe/models/modules.py:174-208
 *   emd_image_loss                      <- l1 + D-SSIM + depth + sky BCE S3Gaussian/utils/loss_utils.py:21-98, train.py:226-363
 *   emd_hexplane_forward / backward     <- HexPlaneField.get_density     S3Gaussian/scene/hexplane.py:18-183
 *   emd_mlp_trunk / emd_mlp_branch      <- feature_out + *_deform heads + dino_head  S3Gaussian/scene/deformation.py:100-185,254-337
 *   emd_temporal_embed_forward/backward <- get_temporal_embed            S3Gaussian/scene/deformation.py:208-221, OmniRe/models/nodes/rigid.py:150-164
 *   emd_deform_input_forward/backward   <- get_embedder + get_deformation OmniRe/models/modules.py:318-366, nodes/deformable.py:35-47
 *   emd_densification_stats             <- add_densification_stats       S3Gaussian/scene/gaussian_model.py:728-730, train.py:403-406
 *   emd_adam_step                       <- optimizer.step()              S3Gaussian/scene/gaussian_model.py:188-201, train.py:428
 *   emd_knn / emd_knn_reverse           <- simple_knn distCUDA2, o3d_knn S3Gaussian/scene/gaussian_model.py:152-181 (create_from_pcd), train.py:326-337
 *   emd_embed_reg_forward / backward    <- weighted_l2_loss_v2 over the neighbour table   S3Gaussian/train.py:326-337
 *   emd_joint_chain_forward / backward, emd_skin_forward / backward
 *                                       <- SMPLTemplate.forward          OmniRe/models/human_body.py:158-181
 *                                          SMPLNodes.transform_means_and_quats  OmniRe/models/nodes/smpl.py:438-532
 *   emd_plane_reg_forward / backward    <- compute_regulation            S3Gaussian/scene/gaussian_model.py:745-784
 *   emd_affine_forward / backward       <- the affine colour correction  OmniRe/models/trainers/base.py:251-258
 *   emd_trainer_loss                    <- compute_losses                OmniRe/models/trainers/base.py:518-620, models/losses.py
 *   emd_vanilla_forward / backward      <- VanillaGaussians.get_gaussians   OmniRe/models/gaussians/vanilla.py:378-414
 *   emd_vanilla_reg_forward / backward  <- VanillaGaussians.compute_reg_loss (the same file)
 *   emd_sh_grad_from_factors            (multi-GPU: rebuilds the SH gradient from all-gathered rank-one factors; no reference counterpart)
 *   emd_compact_rows / emd_scatter_rows (multi-GPU: visibility-compacted gradient rows for 2 / 4 ranks; no reference counterpart)
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions across the ABI; every pointer is a DEVICE
 *     pointer to contiguous fp32/int32 memory unless marked "host".
 *   - the library never allocates or frees device memory: all outputs, scratch and
 *     saved-for-backward state live in caller-owned buffers whose sizes come from
 *     emd_raster_workspace_size().
 *   - every function returns 0 on success, a negative EMD_ERR_* code otherwise;
 *     emd_last_error() returns a thread-local message for the last failure.
 *   - kernels are enqueued on the hipStream_t passed by the caller (as void*).
 *   - matrices use the row-vector convention of S3Gaussian/scene/cameras.py:61-65:
 *     viewmatrix = W2C^T, projmatrix = viewmatrix @ P^T, both row-major 4x4, so that
 *     p_view = [x y z 1] @ viewmatrix.
 */
#ifndef EMD_RASTER_H
#define EMD_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (the deterministic backward extends ABI 30 compatibly -- a new flag bit, two fields at the END of EmdBwdArgs that are read only when the flag
 * is set, new entry points -- so a caller built against the earlier ABI 30 header keeps working and the number stays; the skinning entry points
 * and the plane regularisers at the end of this header are the same kind of extension: new functions and structs only) */
#define EMD_ABI_VERSION 31

/* tile geometry is part of the sort-key contract (tile_id << 32 | depth bits) */
#define EMD_TILE_X 16
#define EMD_TILE_Y 16

enum {
    EMD_OK = 0,
    EMD_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, both/neither of shs & colors...) */
    EMD_ERR_CAPACITY = -2,  /* bin_capacity too small; EmdFwdArgs.num_rendered holds the needed count */
    EMD_ERR_HIP = -3,       /* a HIP runtime call or kernel launch failed */
    EMD_ERR_WORKSPACE = -4, /* a workspace buffer is smaller than emd_raster_workspace_size() reports */
    EMD_ERR_DEPTH_RANGE = -5 /* a visible Gaussian lies more than 65 536 x the near plane away: the three-pass depth sort does not
                                cover it; call again with EMD_FLAG_WIDE_DEPTH_SORT */
};

enum {
    EMD_FLAG_NORMAL   = 1 << 0, /* also composite the view-space normal image (out_normal) */
    EMD_FLAG_MOTION   = 1 << 1, /* fuse the per-actor rigid transform + residual in front of the projection */
    EMD_FLAG_ABSGRAD  = 1 << 2, /* backward also accumulates sum |d L/d mean2D| (gsplat absgrad) */
    EMD_FLAG_NO_SYNC  = 1 << 3, /* never read the duplicate count back to the host; overflow is reported
                                   through EmdStatus.overflow only (graph-capturable path) */
    EMD_FLAG_CLAMP_RGB01 = 1 << 4, /* SH colour clamped to [0,1] (OmniRe, rigid.py:585) instead of >= 0 */
    EMD_FLAG_RAW_PARAMS = 1 << 5,  /* inputs are the raw parameters: scales = log-scales (exp applied here), rotations
                                      un-normalised (normalised here), opacities = logits (sigmoid here); gradients are
                                      returned w.r.t. the raw parameters.  Fuses S3Gaussian/gaussian_renderer/__init__.py:99-101 */
    EMD_FLAG_WIDE_DEPTH_SORT = 1 << 7, /* sort the Gaussians by all 32 depth bits in four passes instead of by the 27 bits above the
                                      near plane in three (needed only when depths exceed 65 536 x the near plane: EMD_ERR_DEPTH_RANGE) */
    EMD_FLAG_SDEV_TANFOV = 1 << 6, /* settings_dev holds two more floats, tanfovx and tanfovy (cameras given as device-resident
                                      intrinsics, OmniRe/models/trainers/base.py:399-400): they replace the by-value fields */
    EMD_FLAG_BWD_WS_CLEAN = 1 << 8, /* backward only (ABI 18): bwd_ws ARRIVES zero-filled (the caller's promise) and is LEFT zero-filled --
                                      the projection backward clears every accumulator row it reads, so a caller that keeps one
                                      workspace across steps pays no 64 N-byte zero fill per backward.  Without the flag the library
                                      clears the workspace itself, as before. */
    EMD_FLAG_BWD_RENDER_ONLY = 1 << 10, /* emd_raster_backward (ABI 21): only the render backward (K7).  With dL_dsh_color set, the clamp-masked
                                      colour gradient of every Gaussian -- the factor of its rank-one dL/dshs -- is extracted from the
                                      accumulator rows right behind it (one small launch), so that a view-parallel step can start the
                                      all-gather of the factors while the projection backward is still to run */
    EMD_FLAG_BWD_PROJECT_ONLY = 1 << 11, /* ... and only the projection backward (K8) on the accumulator rows of such a call: the two halves
                                      of one backward as two calls, with whatever the caller enqueues in between (emd_amd.dp: collectives
                                      on the communication stream).  dL_dsh_color is then left alone (pass NULL). */
    EMD_FLAG_DETERMINISTIC = 1 << 12, /* emd_raster_backward only (ABI 30 extension; the forward ignores it): every output of the backward is a fixed function
                                      of the call's inputs -- no float atomics.  The render backward stores each (quadrant, survivor) row to its own
                                      slot of EmdBwdArgs.det_ws, a stable sort lists the slots per Gaussian and a segmented sum with a pinned
                                      association (EMD_SEG_CHUNK) builds the accumulator rows; the actor-pose gradient goes the same way.  Needs
                                      det_ws (emd_raster_det_workspace_size) on BOTH halves of a two-call backward; refused together with pair_stats */
    EMD_FLAG_KEEP_ALL_PAIRS = 1 << 9 /* (ABI 21) enumerate every tile of upstream's tile rectangle (the 3-sigma square of the largest
                                      eigenvalue): the sorted keys then ARE upstream's (tile << 32 | depth bits) list, entry for entry.
                                      By default a Gaussian enumerates only the tiles of that rectangle which its alpha >= 1/255 bounding
                                      box (half extents sqrt(2 ln(255 o) cov_xx), sqrt(2 ln(255 o) cov_yy)) reaches: the pairs left out are
                                      pairs upstream's render loop skips at every pixel of the tile (its alpha < 1/255 `continue`), so
                                      images, radii and gradients are the same bit for bit and the sorted list is upstream's list with
                                      those entries left out -- same keys, same order, 25 % fewer entries on the street scenes of
                                      BASELINE.json. */
};

/* The 12 fields of GaussianRasterizationSettings (S3Gaussian/gaussian_renderer/__init__.py:49-62), by value. */
typedef struct EmdSettings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float bg[3];
    float scale_modifier;
    float viewmatrix[16];
    float projmatrix[16];
    int32_t sh_degree;      /* active degree 0..3 */
    float campos[3];
    int32_t prefiltered;    /* accepted, ignored (reference always passes False) */
    int32_t debug;          /* !=0: synchronise and check after every stage */
    float near_plane;       /* cull view z <= near_plane; 0.2 for the diff_gauss surface, 0.1 for OmniRe */
} EmdSettings;

/* Per-actor pose row for the fused explicit-motion transform (12 floats, 48 B):
 *   q_mean[4]  unit quaternion (w,x,y,z) rotating local means     rigid.py:499-503
 *   trans[3]   translation incl. learned track offset             rigid.py:519-532
 *   valid      1.0 / 0.0, multiplies opacity                      rigid.py:589-591
 *   q_rot[4]   unit quaternion composed onto local quats (q_mean x track rot offset, rigid.py:562-566)
 */
#define EMD_ACTOR_STRIDE 12
#define EMD_SETTINGS_DEV_FLOATS 38
#define EMD_MAX_EXTRA 2          /* extra colour sets composited by one call (S3Gaussian renders feat_c and feat_f) */

typedef struct EmdMotion {
    const int32_t* actor_id;   /* [N]; -1 = static (identity) */
    const float* actor_pose;   /* [A, EMD_ACTOR_STRIDE] */
    int32_t num_actors;
    const float* residual_dx;  /* [N,3] or NULL: added to the local mean before the rigid transform */
    const float* residual_dq;  /* [N,4] or NULL: added to the local quaternion before normalisation */
} EmdMotion;

/* Small device-side status block written by the forward pass. */
typedef struct EmdStatus {
    uint32_t num_rendered;  /* D = (tile, Gaussian) pairs of the sorted list: the sum over the Gaussians of the tiles their alpha >= 1/255
                               bounding box reaches inside upstream's tile rectangle (ABI 21; with EMD_FLAG_KEEP_ALL_PAIRS: upstream's
                               sum of tiles touched) */
    uint32_t overflow;      /* bit 0: D > bin_capacity; bit 1: depth range beyond the three-pass sort (either: results invalid,
                               the image is the background) */
    uint32_t num_visible;   /* V = Gaussians with radii > 0 */
    uint32_t reserved;      /* internal: visible Gaussians as counted by the depth sort's compacting first pass (== num_visible) */
} EmdStatus;

typedef struct EmdDims {
    int32_t num_gaussians;
    int32_t image_height;
    int32_t image_width;
    int64_t bin_capacity;   /* max (tile, Gaussian) pairs the binning workspace can hold */
    int32_t flags;
    int32_t num_extra;      /* extra colour sets of the call (sizes bwd_ws) */
} EmdDims;

typedef struct EmdFwdArgs {
    EmdSettings s;
    int32_t num_gaussians;
    int32_t sh_coeffs;            /* coefficients stored per Gaussian in shs ([N, sh_coeffs, 3]) */
    int32_t flags;
    int64_t bin_capacity;
    /* inputs */
    const float* means3D;         /* [N,3] (local means when EMD_FLAG_MOTION) */
    const float* shs;             /* [N,sh_coeffs,3] or NULL */
    const float* colors_precomp;  /* [N,3] or NULL; exactly one of shs / colors_precomp */
    const float* opacities;       /* [N] activated */
    const float* scales;          /* [N,3] activated, or NULL */
    const float* rotations;       /* [N,4] (w,x,y,z), or NULL */
    const float* cov3D_precomp;   /* [N,6] or NULL; exactly one of (scales,rotations) / cov3D_precomp */
    EmdMotion motion;
    /* outputs */
    float* out_color;             /* [3,H,W] */
    float* out_depth;             /* [1,H,W] */
    float* out_normal;            /* [3,H,W] (EMD_FLAG_NORMAL) or NULL */
    float* out_alpha;             /* [1,H,W] */
    int32_t* radii;               /* [N] */
    /* caller-owned scratch; kept alive by the caller until backward has run */
    void* geom_ws;  size_t geom_bytes;
    void* bin_ws;   size_t bin_bytes;
    void* img_ws;   size_t img_bytes;
    EmdStatus* status;            /* device, 16 B */
    /* host-side results (filled unless EMD_FLAG_NO_SYNC) */
    int64_t num_rendered;
    int64_t num_visible;
    /* Optional DEVICE copy of the camera-dependent settings, EMD_SETTINGS_DEV_FLOATS floats laid out as
     * bg[3], viewmatrix[16], projmatrix[16], campos[3] (+ tanfovx, tanfovy with EMD_FLAG_SDEV_TANFOV); NULL = use the by-value
     * fields of `s`.  The reference keeps exactly
     * these four on the GPU (`.cuda()` at S3Gaussian/gaussian_renderer/__init__.py:54-59): with this pointer its call site
     * costs no device-to-host copy, so a forward with EMD_FLAG_NO_SYNC never touches the host. */
    const float* settings_dev;
    /* Extra colour sets: the reference's "fine" stage renders the same Gaussians two more times with colors_precomp = ddict["coarse"]["feat"]
     * and ddict["fine"]["feat"] (S3Gaussian/gaussian_renderer/__init__.py:170-201).  With num_extra > 0 those images come out of THIS
     * call: one projection, one sort, one walk over every tile list; out_extra[k] equals, bit for bit, the colour image of a separate
     * call with colors_precomp = colors_extra[k]. */
    int32_t num_extra;                       /* 0 .. EMD_MAX_EXTRA */
    const float* colors_extra[EMD_MAX_EXTRA];  /* [N,3] each */
    float* out_extra[EMD_MAX_EXTRA];           /* [3,H,W] each */
    /* optional second hipStream_t (ABI 18).  With it the forward splits its projection kernel: the geometry half on the call's stream,
     * the colour half (SH colour, clamp bits, colour Jacobian -- read by the compositing kernel only) on aux_stream, beside the binning
     * stage; fork and join are events, i.e. graph edges under stream capture.  The stream must belong to the same device and must not be
     * the call's own; NULL (or debug = 1) keeps everything on one stream.  Same results bit for bit either way. */
    void* aux_stream;
    /* Optional residuals of the SH coefficients (ABI 20), [N,sh_coeffs,3] each or NULL: the colour is evaluated on
     * (shs + shs_residual[0]) + shs_residual[1], added in that order while the rows are staged.  The reference's fine stage forms
     * `shs_final = shs + dshs_coarse + dshs_fine` as two element-wise passes over [N,16,3] before every render
     * (S3Gaussian/scene/deformation.py:468-481); here the sum exists only for the Gaussians that are visible, inside the projection
     * kernel.  dL/dshs of the backward is the gradient of each of the three terms (the sum's Jacobian is the identity). */
    const float* shs_residual[2];
    /* diagnostic (ABI 27): device uint64[6], ADDED to by the compositing kernel's counting instantiation: [0] scan steps (64 list words each),
     * [1] cull steps (64 queued entries each), [2] drain iterations (one entry per 16-pixel row each), [3] entries the rows held, [4] scan -> cull ->
     * drain rounds, [5] waves that ran.  NULL in every training path (the counters are compiled out); num_extra must be 0. */
    uint64_t* loop_stats;
} EmdFwdArgs;

typedef struct EmdBwdArgs {
    EmdSettings s;
    int32_t num_gaussians;
    int32_t sh_coeffs;
    int32_t flags;
    int64_t bin_capacity;
    int64_t num_rendered;         /* D from forward; <0 = read it from status on device */
    /* forward inputs again */
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    EmdMotion motion;
    const int32_t* radii;
    /* forward state (of geom_ws the render backward writes the contributed words, see emd_raster_workspace_size; nothing else in it changes) */
    const void* geom_ws;  size_t geom_bytes;
    const void* bin_ws;   size_t bin_bytes;
    const void* img_ws;   size_t img_bytes;
    const EmdStatus* status;
    /* forward outputs again (the backward pass needs the composited totals per pixel) */
    const float* out_color;       /* [3,H,W] */
    const float* out_depth;       /* [1,H,W] */
    const float* out_normal;      /* [3,H,W] or NULL */
    /* incoming gradients (any may be NULL = zero) */
    const float* dL_dcolor;       /* [3,H,W] */
    const float* dL_ddepth;       /* [1,H,W] */
    const float* dL_dalpha;       /* [1,H,W] */
    const float* dL_dnormal;      /* [3,H,W]  (propagated to the blended normal only) */
    /* scratch for backward, zeroed by the library: one accumulator row per Gaussian, 12 + 4 num_extra floats rounded up to whole 64-byte
     * lines (16, 16, 32 floats for 0, 1, 2 extra sets; the floats behind the payload are never written).  64-byte aligned:
     * EMD_ERR_INVALID otherwise.  Its size comes from emd_raster_workspace_size(). */
    void* bwd_ws;  size_t bwd_bytes;
    /* outgoing gradients (NULL = not wanted) */
    float* dL_dmeans3D;           /* [N,3] */
    float* dL_dmeans2D;           /* [N,3]  x,y in NDC-scaled pixel units (x 0.5 W, 0.5 H), z = 0 */
    float* dL_dmeans2D_abs;       /* [N,2]  (EMD_FLAG_ABSGRAD) */
    float* dL_dshs;               /* [N,sh_coeffs,3], 16-byte aligned when sh_coeffs == 16.  Every element is written by every call, no zero fill by the
                                   * caller: by the projection half alone, except in the one-call default backward with shs and 16 coefficients,
                                   * where the render half zeroes all rows and the projection half stores those of the contributing Gaussians */
    float* dL_dcolors;            /* [N,3] */
    float* dL_dopacities;         /* [N] */
    float* dL_dscales;            /* [N,3] */
    float* dL_drotations;         /* [N,4] */
    float* dL_dcov3D;             /* [N,6] */
    /* motion gradients (EMD_FLAG_MOTION) */
    float* dL_dactor_pose;        /* [A, EMD_ACTOR_STRIDE], zeroed by the library */
    float* dL_dresidual_dx;       /* [N,3] */
    float* dL_dresidual_dq;       /* [N,4] */
    float* dL_dsh_color;          /* [N,3] or NULL: the clamp-masked dL/d(SH colour) of every Gaussian (0 when not visible). With it
                                   * dL_dshs may be NULL: dL/dshs[n][k][c] = basis_k(view direction) * dL_dsh_color[n][c] is rank one and is
                                   * rebuilt (and summed over views) by emd_sh_grad_from_factors -- 12 bytes per Gaussian to exchange
                                   * between GPUs instead of 192 */
    const float* settings_dev;    /* as in EmdFwdArgs (same buffer, kept alive by the caller) */
    /* extra colour sets (see EmdFwdArgs): forward inputs / outputs again, incoming and outgoing gradients; bwd_ws then holds
     * rows of 12 + 4 num_extra floats at the pitch described there (emd_raster_workspace_size with EmdDims.num_extra) */
    int32_t num_extra;
    const float* colors_extra[EMD_MAX_EXTRA];
    const float* out_extra[EMD_MAX_EXTRA];
    const float* dL_dextra[EMD_MAX_EXTRA];        /* [3,H,W] or NULL */
    float* dL_dcolors_extra[EMD_MAX_EXTRA];       /* [N,3] or NULL */
    /* diagnostic (ABI 18; four words since ABI 25): device uint64[4], ADDED to by the render backward: [0] (pixel, list entry) pairs its
     * waves evaluated, [1] pairs that contributed (alpha >= 1/255 in front of the pixel's last contributor), [2] accumulator rows it sent
     * to memory as float atomics (one per (quadrant, survivor) with a non-zero entry), [3] float atomics issued.  NULL in production: the counting
     * instantiation of the kernel is only launched when the pointer is set (plain call only: no extra sets / absgrad / dL_dnormal) */
    uint64_t* pair_stats;
    /* ABI 30 extension, EMD_FLAG_DETERMINISTIC (read ONLY when that flag is set): the workspace of the deterministic backward, emd_raster_det_workspace_size() bytes, 64-byte aligned, caller-owned,
     * never cleared by anybody (no part of it is read before the same call wrote it).  The same buffer on both halves of a two-call backward.
     * EMD_ERR_WORKSPACE when the flag is set and it is missing or short, EMD_ERR_INVALID when misaligned. */
    void* det_ws;  size_t det_bytes;
} EmdBwdArgs;

/* Per-step inputs of a training step that is replayed from ONE hipGraph (ABI 18).  A captured step reads everything that changes
 * from step to step at fixed device addresses; this op fills them from device-resident tables in one launch:
 *   out_row[0..row_floats)  = table[sel[0]]                 e.g. the 38-float settings block of EmdFwdArgs.settings_dev
 *   frame_out[0]            = frames[sel[0]],  t_out[0] = frame / max(num_frames - 1, 1)          (rigid.py:204,241)
 *   k_fine_out[0]           = int(k_min + (k_max - k_min) * clamp(step, 0, k_until) / k_until)    (rigid.py:147-148,194-201)
 *                             with step = steps[sel[0]] (or the row index when steps is NULL)
 * and, for callers that want the device status words of every step without reading them back per step:
 *   status_log[prev_sel[0]] = status[0..4)  (the words the step BEFORE left behind), then prev_sel[0] = sel[0].
 * A call with sel[0] outside [0, rows) only flushes the pending status row.  With next_sel the launch finally sets sel[0] =
 * next_sel[row]: a loop of graph replays walks a schedule of rows without the host touching device memory between replays. */
typedef struct EmdStepSelect {
    int64_t* sel;                    /* device [1]: the row to select; with next_sel it is advanced to next_sel[row] by the launch */
    int32_t rows, row_floats;
    const float* table;              /* [rows, row_floats] */
    float* out_row;                  /* [row_floats] */
    const int32_t* frames;           /* [rows] or NULL */
    int32_t* frame_out;              /* [1] or NULL */
    float* t_out;                    /* [1] or NULL */
    int32_t num_frames;
    int32_t k_min, k_max, k_until;
    const int64_t* steps;            /* [rows] or NULL */
    int32_t* k_fine_out;             /* [1] or NULL */
    const int32_t* status;           /* [4] or NULL */
    int32_t* status_log;             /* [rows, 4] or NULL */
    int64_t* prev_sel;               /* device [1], -1 = nothing pending; or NULL */
    const int64_t* next_sel;         /* [rows] or NULL: successor of every row */
} EmdStepSelect;
int emd_select_step_inputs(const EmdStepSelect* args, void* hip_stream);

int emd_abi_version(void);
const char* emd_last_error(void);

/* out[0..3] = bytes of geom_ws, bin_ws, img_ws, bwd_ws.
 * geom_ws ends with the "contributed" words, one uint32 per Gaussian (a compatible extension of ABI 31: the size reported here grew by 4 N bytes
 * rounded up to 256, no struct changed, and every caller sizes geom_ws through this query).  The forward's projection kernel clears them, the
 * render backward sets word i to 1 when it adds at least one non-zero float to accumulator row i, and the projection backward runs its chain
 * rule for exactly those Gaussians: a Gaussian with radii > 0 that no pixel's gradient reached (occluded behind saturated tiles: more than half
 * of the visible set of a street view) has an all-zero row and exact +0 gradients, written without the loads and the arithmetic.  Under
 * EMD_FLAG_DETERMINISTIC the words are neither written by the backward nor read (radii > 0 decides, as before).  A two-call backward
 * (EMD_FLAG_BWD_RENDER_ONLY, then EMD_FLAG_BWD_PROJECT_ONLY) passes the same geom_ws to both halves, as it always had to. */
int emd_raster_workspace_size(const EmdDims* dims, size_t out[4]);

int emd_raster_forward(EmdFwdArgs* args, void* hip_stream);
int emd_raster_backward(const EmdBwdArgs* args, void* hip_stream);

/* ABI 31 extension (a new entry point only, so the number stays).  Host only, for tests: the slice [out[0], out[1]) of `count` 16-byte elements
 * that workgroup `block` of the `grid` workgroups of the render backward zeroes when that kernel clears dL_dshs for the projection backward
 * (csrc/common.h, emd_fill_slice -- the function the kernel calls).  Slices are disjoint, ascending and cover [0, count) exactly; every slice
 * but the last non-empty one is a multiple of 64 elements long.  EMD_ERR_INVALID for grid == 0, block >= grid or a NULL out. */
int emd_backward_fill_slice(uint64_t count, uint32_t grid, uint32_t block, uint64_t out[2]);

/* ---- ABI 30 extension: the deterministic backward (opt-in, EMD_FLAG_DETERMINISTIC) ------------------------------------------------------------
 * Bytes of EmdBwdArgs.det_ws for dims (num_gaussians N, bin_capacity C, num_extra x).  R = 4 max(C, 1) contribution slots (one per quadrant
 * and list entry: the worst case; only the slots below 4 D are ever touched), n = max(N, 1), p = the accumulator row pitch in floats
 * (16, 16, 32 for x = 0, 1, 2), up(b) = b rounded up to 256:
 *     sort(m, g) = 5 up(4 m) + up(4 * 512 ceil(m / 2048)) + up(8 g * 2 ceil(m / EMD_SEG_CHUNK))
 *                  raw keys and two ping-pong pairs, the histograms, the fp64 chunk sums of the segmented sum (g doubles each)
 *     bytes      = up(4 R p) + sort(R, 12 + 4 x <= 16 ? 16 : 32) + up(64) + up(48 n) + sort(n, 16) + 256
 *                  contribution rows, the render sort, the count words, the [N, 12] pose rows, the pose sort
 * The layout is emd_carve_det of csrc/det_backward.h.  Nothing in it needs clearing. */
int emd_raster_det_workspace_size(const EmdDims* dims, size_t* bytes);
/* Byte offsets inside det_ws, for tests and profiles: [0] contribution rows  [1] / [2] the two key buffers and [3] / [4] the two slot buffers of
 * the render sort  [5] the count words (uint32: [0] slots in use = 4 D, [1] contributions the sort kept, [2] actor-bound visible points)
 * [6] the [N, 12] pose rows  [7] / [8] key and [9] / [10] point-index buffers of the pose sort  [13] / [14] the raw keys of the two sorts;
 * out[11] = which pair (0 / 1) holds the sorted render lists after a backward, out[12] the same for the pose lists with num_actors actors */
int emd_raster_det_layout(const EmdDims* dims, int32_t num_actors, size_t out[15]);

/* ---- ABI 30: the gradient of the camera (opt-in; camera-pose optimisation) --------------------------------------------------------
 * dL/d(viewmatrix[16], projmatrix[16], campos[3]) of one call, 35 floats laid out as the settings block is (viewmatrix as
 * EmdSettings.viewmatrix: V[4 k + r], translation at 12..14).  Every entry the projection reads is a free variable; the entries it never
 * reads (V[3], V[7], V[11], V[15], the z column P[4 k + 2]) receive an exact 0.  The chain rule back to a camera pose is the caller's.
 * The backward is then issued in its two halves with this call in between, all on one stream:
 *     backward with EMD_FLAG_BWD_RENDER_ONLY  ->  backward_camera  ->  backward with EMD_FLAG_BWD_PROJECT_ONLY
 * on the same EmdBwdArgs: it reads the accumulator rows the render half left in bwd_ws and changes none of them (the projection half
 * still consumes them, and hands them back zeroed under EMD_FLAG_BWD_WS_CLEAN).  All 35 outputs are written by every call (no zero fill
 * by the caller; num_gaussians == 0 gives 35 zeros).  The sum is deterministic: per-workgroup rows in `workspace` (the size the first
 * function reports, 16-byte aligned; EMD_ERR_WORKSPACE when smaller), added in a fixed order in double precision -- no float atomics.
 * The normal image's dependence on the view matrix is not covered: a non-NULL dL_dnormal is refused with EMD_ERR_INVALID.
 * No gradient for tanfov, the intrinsics behind projmatrix, or bg. */
int emd_camera_grad_workspace_size(int32_t num_gaussians, size_t* bytes);
int emd_raster_backward_camera(const EmdBwdArgs* args, float* dL_dcamera /*[35], device*/, void* workspace, size_t workspace_bytes,
                               void* hip_stream);

/* Copy binning state out for parity tests: sorted keys (tile<<32 | depth bits), sorted Gaussian ids, the quadrant mask of every
 * entry (bit q = qy * 2 + qx: the Gaussian's alpha >= 1/255 footprint reaches the 8x8 quadrant q of the tile; ABI 21),
 * per-tile [start,end) ranges.  Any output may be NULL.  keys / ids / quad_masks hold num_entries = EmdStatus.num_rendered entries.
 * The sort itself moves (tile id, Gaussian id) pairs of Gaussians pre-ordered by depth; the 64-bit keys of the
 * reference are rebuilt here from the tile id and the depth bits kept per Gaussian in geom_ws. */
int emd_raster_export_binning(const EmdDims* dims, const void* geom_ws, size_t geom_bytes, const void* bin_ws, size_t bin_bytes,
                              int64_t num_entries, uint64_t* keys, uint32_t* ids, uint32_t* ranges /*[T,2]*/,
                              uint32_t* quad_masks, void* hip_stream);

/* Copy per-Gaussian projection state out for parity tests.  Any output may be NULL. */
int emd_raster_export_geometry(const EmdDims* dims, const void* geom_ws, size_t geom_bytes,
                               float* means2D /*[N,2]*/, float* depths /*[N]*/, float* conic_opacity /*[N,4]*/,
                               float* rgb /*[N,3]*/, float* normal /*[N,3]*/, uint32_t* tiles_touched /*[N]*/,
                               void* hip_stream);

/* Copy the contributed words of geom_ws (emd_raster_workspace_size) out for tests and counts: contributed[i] = 1 when the last render backward on
 * this geom_ws added to the accumulator row of Gaussian i, 0 otherwise (all 0 between a forward and its backward).  dims: num_gaussians only. */
int emd_raster_export_contributed(const EmdDims* dims, const void* geom_ws, size_t geom_bytes, uint32_t* contributed /*[N]*/, void* hip_stream);

/* Stand-alone explicit-motion transform (same arithmetic as the fused path):
 *   world_mean = R(q_mean[a]) (mean + dx) + trans[a];  world_quat = q_rot[a] (x) normalize(quat + dq);
 *   opacity_out = opacity * valid[a].  Outputs may be NULL. */
int emd_motion_forward(int32_t n, const float* means, const float* quats, const float* opacities,
                       const EmdMotion* motion, float* world_means, float* world_quats, float* opacities_out,
                       void* hip_stream);
int emd_motion_backward(int32_t n, const float* means, const float* quats, const float* opacities,
                        const EmdMotion* motion, const float* dL_dworld_means, const float* dL_dworld_quats,
                        const float* dL_dopacities_out, float* dL_dmeans, float* dL_dquats, float* dL_dopacities,
                        float* dL_dactor_pose /*[A,12] zeroed here*/, float* dL_dresidual_dx, float* dL_dresidual_dq,
                        void* hip_stream);

/* ---- ABI 30 extension: the deterministic motion backward (opt-in; an entry point of its own, so that emd_motion_backward and its kernel are unchanged) ----
 * emd_motion_backward with one difference: dL_dactor_pose is not accumulated with float atomics.  Every actor-bound point (actor_id >= 0) stores its
 * twelve floats as row i of an [n, 12] buffer, a stable compacting sort lists the points per actor, and the lists are added with the association of
 * emd_segmented_row_sum.  Contract: an actor's pose gradient is the sum of its points' rows in ASCENDING POINT INDEX -- chunks of EMD_SEG_CHUNK = 512,
 * each summed in fp64 in ascending order from 0.0, the chunk sums added in ascending order in fp64 from 0.0, one rounding to fp32.  Actors without a
 * point get zeros (dL_dactor_pose is zeroed here).  Nothing of it depends on workgroup order, the stream, other work on the device, or eager execution
 * against hipGraph replay; no kernel of the mode uses an atomic or a device-scope fence.  The per-point outputs are those of emd_motion_backward, bit for
 * bit.  Every argument check of emd_motion_backward applies; in addition 4 n <= 2^32 - 1 - 2048 (EMD_ERR_INVALID otherwise).
 * det_ws: caller-owned, 256-byte aligned, never cleared; missing, misaligned or shorter than emd_motion_det_workspace_size(n) is EMD_ERR_WORKSPACE,
 * decided before anything is launched.  When dL_dactor_pose is NULL no workspace is needed (det_ws may be NULL).
 * Bytes of det_ws, m = max(n, 1), up(b) = b rounded up to 256, sort(m, g) as for emd_raster_det_workspace_size:
 *     bytes = up(48 m) + sort(m, 16) + up(64) + 256
 *             the [n, 12] pose rows, the sort by actor with the chunk sums, the count words
 * emd_motion_det_workspace_size is host-only and returns 0 for an n outside the limit.  emd_motion_det_workspace_offsets gives the byte offsets inside
 * det_ws of what a call with num_actors actors leaves there, for tests and profiles: out[0] the pose rows, [1] the raw keys (actor id of every point,
 * 0xFFFFFFFF = static), [2] the sorted keys and [3] the sorted point indices -- the ping-pong pair that holds the result for this num_actors --,
 * [4] the count words (uint32 [0] = points the sort kept), out[5] = the total, as emd_motion_det_workspace_size reports it. */
size_t emd_motion_det_workspace_size(int32_t n);
int emd_motion_det_workspace_offsets(int32_t n, int32_t num_actors, size_t out[6]);
int emd_motion_backward_det(int32_t n, const float* means, const float* quats, const float* opacities,
                            const EmdMotion* motion, const float* dL_dworld_means, const float* dL_dworld_quats,
                            const float* dL_dopacities_out, float* dL_dmeans, float* dL_dquats, float* dL_dopacities,
                            float* dL_dactor_pose /*[A,12] zeroed here*/, float* dL_dresidual_dx, float* dL_dresidual_dq,
                            void* det_ws, size_t det_bytes, void* hip_stream);

/* Spherical harmonics colour (no +0.5, no clamp): rgb = SH_deg(dirs / |dirs|) . coeffs */
int emd_sh_forward(int32_t n, int32_t degree, int32_t sh_coeffs, const float* dirs /*[N,3]*/,
                   const float* coeffs /*[N,K,3]*/, float* rgb /*[N,3]*/, void* hip_stream);
int emd_sh_backward(int32_t n, int32_t degree, int32_t sh_coeffs, const float* dirs, const float* coeffs,
                    const float* dL_drgb, float* dL_dcoeffs, float* dL_ddirs /*or NULL*/, void* hip_stream);

/* Dense SH-coefficient gradient from per-view factors (view-parallel data parallelism):
 *   dL_dshs[n][k][c] = scale * sum_v basis_k(normalize(world_mean_n - campos[v])) * sh_color_grads[v][n][c]      k < (degree+1)^2
 * with world_mean_n the mean after the explicit-motion transform (motion may be NULL: static scene).  Every rank gathers
 * the [N,3] factors and the camera centres of all views and rebuilds the same dense, averaged gradient locally.
 * pose_per_view != 0: the views belong to different timestamps (six cameras on eight ranks), motion->actor_pose is then
 * [V, A, EMD_ACTOR_STRIDE] -- one gathered pose table per view -- and an actor's Gaussians are placed per view. */
int emd_sh_grad_from_factors(int32_t n, int32_t num_views, int32_t degree, int32_t sh_coeffs, const float* means3D,
                             const EmdMotion* motion, int32_t pose_per_view, const float* campos /*[V,3]*/,
                             const float* sh_color_grads /*[V,N,3]*/, float scale, float* dL_dshs /*[N,sh_coeffs,3]*/,
                             void* hip_stream);

/* Visibility-compacted rows for the view-parallel gradient exchange (ABI 25; no reference counterpart -- the
 * reference trains one view per step on one GPU, S3Gaussian/train.py:203).  A view's gradient is zero for every Gaussian it does not see:
 * a rank sends (index, values) rows of its visible Gaussians with an all-gather instead of all-reducing dense [N, .] tensors, and every
 * rank adds the gathered rows into a dense buffer in rank order (a fixed order of float additions: replicas stay bit-identical).
 *
 * emd_compact_rows: rows is uint32 [(1 + capacity) * row_words], row_words = 1 + sum(widths).  rows[0 .. row_words) is the header
 * (count of data rows, overflow flag: more visible Gaussians than capacity -- the surplus rows are dropped and the receiver must not
 * trust the step -- then zeros); data row j = (Gaussian index, the widths[k] floats of sources[k][index] for k = 0 .. num_sources - 1) for
 * the Gaussians with radii > 0, in no particular order.  counter: one device uint32 of scratch.
 * emd_scatter_rows: one gathered view: for j < header.count: dests[k][index] = (add ? dests[k][index] : 0) + scale * value.  Indices are
 * unique within a view (no atomics); launch the views one after the other.  overflow_out (optional device uint32) gets bit 0 set when the
 * header carries the overflow flag. */
#define EMD_ROW_SOURCES 4
int emd_compact_rows(int32_t n, const int32_t* radii, int32_t num_sources, const float* const* sources, const int32_t* widths,
                     int64_t capacity, uint32_t* rows, uint32_t* counter, void* hip_stream);
int emd_scatter_rows(const uint32_t* rows, int64_t capacity, int32_t num_dst_rows, int32_t num_dests, float* const* dests,
                     const int32_t* widths, int32_t add, float scale, uint32_t* overflow_out, void* hip_stream);

/* Densification statistics of one view (the per-step part): for every Gaussian with radii > 0
 * grad_accum += |dL_dmeans2D.xy|, denom += 1, max_radii2D = max(max_radii2D, radii), in place -- gaussian_model.py:728-730 and
 * train.py:403-406 without their boolean-mask indexing (a host sync per step).  Any of the three outputs may be NULL. */
int emd_densification_stats(int32_t n, const int32_t* radii, const float* dL_dmeans2D /*[N,3]*/, float* grad_accum /*[N]*/,
                            float* denom /*[N]*/, float* max_radii2D /*[N]*/, void* hip_stream);

/* Per-frame actor pose table, training branch of RigidNodes.transform_means / transform_quats
 * (OmniRe/models/nodes/rigid.py:499-503,519-532,547-566): pose[a] = (normalize(q_f[a]), t_f[a] + dt[a], valid[a],
 * normalize(q_f[a] (x) dq[a])).  q_f [A,4] raw pose quaternions of the frame, t_f [A,3], valid [A] bytes or NULL,
 * dt [A,3] / dq [A,4] learned track offsets or NULL (NaN rows are skipped as the reference does).
 * frame_dev (optional): a DEVICE int32 holding the frame index; q_f / t_f / valid (and dL_dq_f / dL_dt_f) are then the whole
 * [F, A, .] tables and the row is selected on the device -- the call is then replayable from a hipGraph with a new frame. */
int emd_actor_pose_forward(int32_t num_actors, const float* q_f, const float* t_f, const uint8_t* valid, const float* dt,
                           const float* dq, float* pose /*[A,12]*/, const int32_t* frame_dev, void* hip_stream);
int emd_actor_pose_backward(int32_t num_actors, const float* q_f, const float* dt, const float* dq, const float* dL_dpose,
                            float* dL_dq_f, float* dL_dt_f, float* dL_ddt /*or NULL*/, float* dL_ddq /*or NULL*/,
                            const int32_t* frame_dev, void* hip_stream);

/* L1 photometric loss of the training step (S3Gaussian/utils/loss_utils.py:21-22, train.py:226):
 * loss[0] = mean |a - b| over n elements, grad[i] = sign(a[i] - b[i]) / n (grad may be NULL).  One launch.
 * b == NULL: loss[0] = mean |a| -- the residual regularisers of the fine stage (the L1 norms of dx / do / dshs, S3Gaussian/train.py);
 * emd_abs_mean_backward writes their gradient sign(x[i]) * g[0] / n with the upstream gradient g read on the device. */
int emd_l1_loss(int64_t n, const float* a, const float* b, float* loss /*[1]*/, float* grad /*[n] or NULL*/, void* hip_stream);
/* ABI 25.  The same with a caller-kept scratch table (EMD_L1_SCRATCH_WORDS 4-byte words, 8-byte aligned, ZERO at the first call and left zero by
 * every call; used by one stream at a time): every workgroup publishes its partial sum there as one 8-byte {value, tag} granule, workgroup 0
 * adds them in workgroup order and writes `loss` -- no zero fill of `loss` in front of the kernel (a launch of its own: 4.6 us of a 1.3 ms
 * step), and a sum that does not depend on the order of float atomics.  scratch == NULL is emd_l1_loss. */
#define EMD_L1_SCRATCH_WORDS 1024
int emd_l1_loss_ws(int64_t n, const float* a, const float* b, float* loss /*[1]*/, float* grad /*[n] or NULL*/, uint32_t* scratch /*[EMD_L1_SCRATCH_WORDS]*/,
                   void* hip_stream);
int emd_abs_mean_backward(int64_t n, const float* x, const float* g /*[1], device*/, float* grad /*[n]*/, void* hip_stream);
/* ABI 20.  The backward of a PAIR of regularised residuals that also feed the renderer (dshs_coarse / dshs_fine of the fine stage,
 * S3Gaussian/train.py:238-310 with scene/deformation.py:468-481): grad_a[i] = up_a[i] + sign(x_a[i]) g_a[0] / n, likewise b, in one
 * pass; up_a / up_b (the renderer's dL/dshs, usually one tensor: read once when the pointers are equal) and g_a / g_b may be NULL (= 0). */
int emd_residual_l1_backward(int64_t n, const float* up_a, const float* up_b, const float* x_a, const float* x_b, const float* g_a /*[1], device*/,
                             const float* g_b /*[1], device*/, float* grad_a /*[n]*/, float* grad_b /*[n]*/, void* hip_stream);

/* The activations exactly as EMD_FLAG_RAW_PARAMS applies them (exp, F.normalize, sigmoid); any pair may be NULL. */
int emd_activations_forward(int32_t n, const float* log_scales, float* scales, const float* raw_quats, float* quats,
                            const float* opacity_logits, float* opacities, void* hip_stream);

/* Per-stage device timing with HIP events recorded on the caller's stream around each stage (bench.py's roofline
 * leg).  Stages: see emd_profile_stage_name().  emd_profile_read synchronises on the recorded events, adds the
 * elapsed milliseconds and launch counts per stage into ms[]/count[] (up to max_stages entries) and clears the
 * recorded events; returns the number of stages. */
#define EMD_PROF_STAGES 8
int emd_profile_enable(int on);
int emd_profile_read(double* ms, int64_t* count, int max_stages);
const char* emd_profile_stage_name(int stage);


/* ==== widening rows of the scope table, each behind the reference's own module surface ==== */

/* ---- sky cube map + final blend -------------------------------------------------
 * Replaces S3Gaussian/scene/sky_cubemap.py:41-87 (SkyCubeMap.forward: get_rays_torch, mask, nvdiffrast dr.texture
 * 'linear'/'cube', clamp) with the blend of gaussian_renderer/__init__.py:299-301, and OmniRe/models/modules.py:174-208
 * (EnvLight.forward) with the blend of models/trainers/base.py:491-497. */
#define EMD_SKY_CLAMP01     1   /* clamp the looked-up colour to [0,1] (S3G) */
#define EMD_SKY_BLEND_S3G   2   /* out = fg * acc + sky * (1 - acc) */
#define EMD_SKY_BLEND_ADD   4   /* out = fg + sky * (1 - acc) (OmniRe) */
#define EMD_SKY_INTERLEAVED 8   /* images are [P,3]; default planar [3,P] */

typedef struct EmdSkyArgs {
    int32_t height, width;      /* P = height * width pixels (a flat list of directions: height 1) */
    int32_t resolution;         /* cube faces are resolution x resolution texels */
    int32_t flags;              /* EMD_SKY_* */
    const float* cube;          /* [6,res,res,3] faces +x,-x,+y,-y,+z,-z (OpenGL orientation) */
    const float* dirs;          /* [P,3] lookup directions in the cube's frame, or NULL: pinhole rays below */
    float Kinv[9], R[9], T[3];  /* row-major inverse intrinsics, w2c rotation, w2c translation: get_rays_torch(H,W,K,R,T) */
    const float* jitter;        /* [P,2] sub-pixel offsets (training: U[0,1)), or NULL: pixel centres (+0.5) */
    const float* acc;           /* [P] foreground opacity ("weight"), or NULL */
    float mask_threshold;       /* with acc: texture sampled where (1 - acc) > threshold (S3G: 1e-3), else sky = fill; <0: always */
    float fill;                 /* sky colour of masked-out pixels */
    const float* fg;            /* foreground image for the blend, or NULL */
    float* sky;                 /* out: sky colour, or NULL */
    float* out;                 /* out: blended image, or NULL */
    const float* camera_dev;    /* optional (ABI 21): Kinv[9], R[9], T[3] on the DEVICE (21 floats) -- they replace the by-value fields, so a pass
                                   recorded into a hipGraph can serve every camera of a rig (emd_amd.StepInputs) */
} EmdSkyArgs;

typedef struct EmdSkyBwdArgs {
    EmdSkyArgs f;               /* the forward arguments (sky / out unused) */
    const float* dL_dout;       /* gradient of the blended image, or NULL */
    const float* dL_dsky;       /* gradient of the sky colour output, or NULL */
    float* dL_dcube;            /* [6,res,res,3], zeroed here and accumulated with float atomics; or NULL */
    float* dL_dacc;             /* [P] through the blend only (the mask is not differentiated), or NULL */
    float* dL_dfg;              /* like fg, or NULL */
} EmdSkyBwdArgs;

int emd_sky_forward(const EmdSkyArgs* args, void* hip_stream);
int emd_sky_backward(const EmdSkyBwdArgs* args, void* hip_stream);

/* ---- ABI 30 extension: the deterministic sky backward (opt-in; an entry point of its own, so that EmdSkyBwdArgs, emd_sky_backward and its kernel are
 * unchanged).  emd_sky_backward with one difference: dL_dcube is not accumulated through LDS windows and float atomics.  Tap k (0..3, the order of the
 * bilinear footprint: (u0,v0), (u1,v0), (u0,v1), (u1,v1)) of pixel p stores the three floats w_k * dL/d(sky colour) as a row at slot e = k P + p, with
 * P = height * width and p the row-major pixel index (for a direction list: the list index); a stable compacting sort lists the slots per texel and the
 * lists are added with the association of emd_segmented_row_sum.  A tap contributes when its pixel is sampled (mask / threshold) and its weight is not
 * zero (a cube corner's missing fourth tap has weight zero); a row of zeros is still a contribution.
 * Contract: a texel's gradient is the sum of its contributions in ASCENDING (k, p) ORDER -- chunks of EMD_SEG_CHUNK = 512, each summed in fp64 in
 * ascending order from 0.0, the chunk sums added in ascending order in fp64 from 0.0, one rounding to fp32.  Texels without a contribution are +0.0
 * (dL_dcube is zeroed here).  Nothing of it depends on workgroup order, the stream, other work on the device, or eager execution against hipGraph
 * replay; no kernel of the mode uses an atomic or a device-scope fence.  dL_dfg and dL_dacc are those of emd_sky_backward, bit for bit.  Both call
 * shapes are served: the pinhole image (planar or interleaved, with or without jitter and camera_dev) and the direction list (height 1).
 * Every argument check of emd_sky_backward applies; in addition 4 P <= 2^32 - 1 - 2048 and 6 resolution^2 <= 2^30 (EMD_ERR_INVALID otherwise).
 * det_ws: caller-owned, 256-byte aligned, never cleared; missing, misaligned or shorter than emd_sky_det_workspace_size(P) is EMD_ERR_WORKSPACE,
 * decided before anything is launched.  When dL_dcube is NULL no workspace is needed (det_ws may be NULL).
 * Bytes of det_ws, m = 4 max(P, 1) slots, up(b) = b rounded up to 256, sort(m, g) as for emd_raster_det_workspace_size:
 *     bytes = up(16 m) + sort(m, 16) + up(64) + 256
 *             the rows at a pitch of 4 floats (three channels and a pad: one 16-byte store), the sort by texel with the chunk sums, the count words
 * emd_sky_det_workspace_size is host-only and returns 0 for a P outside the limit.  emd_sky_det_workspace_offsets gives the byte offsets inside det_ws
 * of what a call leaves there, for tests and profiles: out[0] the rows, [1] the raw keys (flat texel index of every slot, 0xFFFFFFFF = no contribution),
 * [2] the sorted keys and [3] the sorted slots -- the ping-pong pair that holds the result for this resolution --, [4] the count words (uint32 [0] =
 * slots the sort kept), out[5] = the total, as emd_sky_det_workspace_size reports it. */
size_t emd_sky_det_workspace_size(int64_t num_pixels);
int emd_sky_det_workspace_offsets(int64_t num_pixels, int32_t resolution, size_t out[6]);
int emd_sky_backward_det(const EmdSkyBwdArgs* args, void* det_ws, size_t det_bytes, void* hip_stream);

/* ---- image-loss tail -----------------------------------------------------------------
 * loss = L1 + lambda_depth * depth L2 + lambda_dssim * (1 - SSIM 11x11) + lambda_sky * sky BCE, with the gradients with
 * respect to the rendered image, depth and weight in the planar layouts emd_raster_backward consumes.  Replaces
 * S3Gaussian/utils/loss_utils.py:21-98 (compute_depth "l2", l1_loss, ssim) as used in S3Gaussian/train.py:226-363.
 * The depth term is on when depth / gt_depth are given and lambda_depth != 0, the sky term when weight / sky_mask are given and lambda_sky > 0.
 * Two rules about the gradients:
 *   - every requested gradient (pointer not NULL) is written in full by the call.  One whose term is off is +0 everywhere, as is dL_ddepth
 *     without a single valid lidar pixel: the caller may hand over uninitialised memory.  An output passed as NULL is not computed, and the
 *     other outputs are bit for bit what they are when all are requested;
 *   - the sky term is applied only when sky_mask holds at least one sky pixel (train.py:360).  Without one its loss is 0 and dL_dweight is +0
 *     everywhere, whichever other gradients are requested and whatever lambda_dssim is. */
typedef struct EmdLossArgs {
    int32_t height, width;
    const float* image;        /* [3,H,W] rendered */
    const float* gt;           /* [3,H,W] target */
    const float* depth;        /* [H,W] rendered depth, or NULL (no depth term) */
    const float* gt_depth;     /* [H,W] lidar depth (0 where absent) */
    const float* mask;         /* [H,W] multiplies both depths (train.py: ~sky_mask), or NULL = ones */
    const float* weight;       /* [H,W] rendered opacity, or NULL (no sky term) */
    const uint8_t* sky_mask;   /* [H,W] 1 = sky */
    float lambda_dssim, lambda_depth, lambda_sky, max_depth;   /* reference: 0.2, 0.5, 0.05, 80 */
    float* losses;             /* out [5]: total, l1, ssim, depth, sky */
    float* dL_dimage;          /* out [3,H,W] or NULL */
    float* dL_ddepth;          /* out [H,W] or NULL */
    float* dL_dweight;         /* out [H,W] or NULL */
} EmdLossArgs;

size_t emd_image_loss_workspace(int height, int width);
int emd_image_loss(const EmdLossArgs* args, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- HexPlane feature lookup -------------------------------------------------------------
 * Replaces HexPlaneField.get_density / interpolate_ms_features (S3Gaussian/scene/hexplane.py:18-110,150-183): for every
 * scale the product over the six coordinate planes (xy, xz, xt, yz, yt, zt) of a bilinear, align_corners, border-padded
 * grid_sample, concatenated over scales.  Planes are passed CHANNEL-LAST: [res_h][res_w][C]. */
#define EMD_HEX_MAX_SCALES 8
typedef struct EmdHexArgs {
    int32_t num_points, channels, num_scales;
    int32_t times_broadcast;                     /* (ABI 24) non-zero: `times` holds ONE timestamp, shared by all points */
    int32_t res[EMD_HEX_MAX_SCALES][4];          /* per scale: resolution along x, y, z, t */
    const float* planes[EMD_HEX_MAX_SCALES][6];  /* per scale: planes of the pairs (0,1),(0,2),(0,3),(1,2),(1,3),(2,3), [res[b]][res[a]][C] */
    const float* pts;                            /* [N,3] */
    const float* times;                          /* [N], or one float with times_broadcast */
    float aabb[6];                               /* aabb[0] (3 floats) then aabb[1] (3 floats), as HexPlaneField stores them */
    float* out;                                  /* [N, num_scales * C] (forward) */
    const int32_t* order;                        /* [N] a permutation of the points, or NULL: the order the kernels visit them in.
                                                    A spatially coherent one (e.g. Morton order of pts) lets the backward
                                                    aggregate the plane gradients in LDS before they reach HBM; results are
                                                    the same up to the order of the float sums. */
    float* time_tables;                          /* (ABI 23) NULL, or scratch of C * sum over scales of (res_x + res_y + res_z) floats.  Non-NULL is
                                                    the caller's PROMISE that every timestamp equals times[0] (one frame per step: always, in
                                                    training): emd_hexplane_forward then blends the two time rows of the planes (x,t), (y,t),
                                                    (z,t) into 1-D tables once per call and reads two taps instead of four on those planes --
                                                    18 instead of 24 tap rows per point and scale.  Same values up to rounding ((1-fx) [(1-ft) nw
                                                    + ft sw] + fx [...] instead of the four-term sum).  The backward does not use it. */
} EmdHexArgs;

typedef struct EmdHexGrads {
    const float* dL_dout;                        /* [N, num_scales * C] */
    float* dL_dplanes[EMD_HEX_MAX_SCALES][6];    /* channel-last like planes; ZEROED BY THE CALLER, accumulated with float atomics (EMD_HEX_FLAG_DETERMINISTIC: written per texel); may be NULL */
    float* dL_dpts;                              /* [N,3] or NULL */
    float* dL_dtimes;                            /* [N] or NULL (reaches the reference's time_offset parameter, deformation.py:325-328) */
    /* Optional per-plane pass for the fine scales (ABI 19; needs args->order and 16 or 32 channels).  On the scales named by
     * defer_mask a run of 256 points that is compact in 3-D still spans tens of cells of a SPATIAL plane and puts ~1 tap into a cell,
     * so nothing aggregates and every tap row is a global atomic.  With the three extra orders below the backward instead writes, per
     * point and spatial plane, the 128-byte row dL/d(interpolated plane value) into defer_rows at the point's position in THAT
     * plane's order, and a second launch walks each plane in its own order -- runs that are compact in the plane's two coordinates
     * share cells -- and adds the taps through LDS windows.  Any permutations give the same sums (up to float rounding); all of
     * order2d / pos2d / defer_rows must be non-NULL when defer_mask != 0. */
    const int32_t* order2d[3];                   /* [N] each: visiting order of the planes xy, xz, yz */
    const int32_t* pos2d[3];                     /* [N] each: the inverse permutations, pos2d[p][order2d[p][i]] = i */
    float* defer_rows;                           /* scratch of popcount(defer_mask) * 3 * N * C + 6 * N floats (the rows, then the planes' coordinates); written and read by the call */
    uint32_t defer_mask;                         /* bit s set: the spatial planes of scale s go through the per-plane pass */
    uint32_t flags;                              /* EMD_HEX_FLAG_*; 0 from every caller that knew the field as `reserved` */
    float* dL_dtime_sum;                         /* (ABI 24) NULL, or one float ZEROED BY THE CALLER that receives sum_n dL/dtimes[n] (float atomics, one per
                                                    workgroup): the gradient of a broadcast timestamp -- S3Gaussian's time_offset parameter,
                                                    deformation.py:325-328 -- without the [N] gradient and its reduction; used when dL_dtimes is NULL.
                                                    With EMD_HEX_FLAG_DETERMINISTIC the call WRITES the float (the pinned sum below) instead of adding to it */
    /* ABI 30 extension, read only with EMD_HEX_FLAG_DETERMINISTIC (below) */
    void* det_ws;  size_t det_bytes;             /* emd_hexplane_det_workspace_size() bytes, caller-owned, 256-byte aligned, never cleared; needed when a plane
                                                    gradient or dL_dtime_sum is asked for */
    uint32_t det_keep_plane;                     /* 0: none; 1 + 6 s + p: plane p of scale s is processed LAST, so that after the call det_ws still holds its
                                                    rows, sorted keys and sorted slots (emd_hexplane_det_workspace_offsets).  Changes no output bit: the order
                                                    in which planes are processed is part of no sum.  For tests and profiles */
} EmdHexGrads;

int emd_hexplane_forward(const EmdHexArgs* args, void* hip_stream);
int emd_hexplane_backward(const EmdHexArgs* args, const EmdHexGrads* grads, void* hip_stream);

/* ---- ABI 30 extension: the deterministic HexPlane backward (opt-in, EmdHexGrads.flags) -----------------------------------
 * With the flag every output of ONE emd_hexplane_backward call -- every dL_dplanes[s][p], dL_dpts, dL_dtimes, dL_dtime_sum -- is a fixed function
 * of that call's inputs: workgroup scheduling, the stream, other work on the device, eager execution against hipGraph replay have no influence, and
 * EmdHexArgs.order and EmdHexGrads.order2d / pos2d / defer_rows / defer_mask are ignored.  No float atomics, no LDS adds shared between points.
 *   Plane (s, p), W x H texels: a CONTRIBUTION is one (point n, tap k) pair, k = 0..3 for the taps (x0,y0), (x1,y0), (x0,y1), (x1,y1).  Its
 *     destination is the tap's texel y W + x, the clamped neighbour included (at the border x1 == x0: several taps of a point then share a texel
 *     and stay separate contributions, weight-0 rows included).  Its value is the C-float row gi w_k the default backward would add; every row is
 *     stored, zeros too (no gi != 0 skip).  A texel's gradient is the sum of its contributions in ascending (k, n) order -- tap-major, then point
 *     index -- with the association of emd_segmented_row_sum: chunks of EMD_SEG_CHUNK = 512, each summed in fp64 in ascending order from 0.0, the
 *     chunk sums added in ascending order from 0.0, one rounding to fp32.  Texels without a contribution keep the caller's zeros.
 *   dL_dpts, dL_dtimes: formed by the point's own C lanes -- over scales, then planes, in registers, then a fixed xor-shuffle tree over the lanes.
 *   dL_dtime_sum: the emd_segmented_row_sum of the per-point values in ascending n, one run under one key; written, not added to.
 * Layout: per plane with a gradient, on the caller's stream: a row kernel (lane = channel) stores the four rows of point n at slots e = k N + n of
 * a [4 N][C] buffer and the texel as key[e]; the stable compacting radix sort lists the slots per texel (ceil(log2(W H)) key bits in passes of at
 * most nine; stable, so ascending e inside a texel = ascending (k, n)); the segmented row sum writes dL_dplanes[s][p].  The workspace is reused
 * from plane to plane.  One more launch forms dL_dpts / dL_dtimes / the time column.
 * Accepts the channel counts of the default path up to 32 (the segmented sum's row width): more is EMD_ERR_INVALID; the flag without a large
 * enough det_ws is EMD_ERR_WORKSPACE (when a plane gradient or dL_dtime_sum is asked for); both are decided before anything is launched.
 *
 * Bytes of det_ws, n = max(num_points, 1), C = channels, g = (C <= 16 ? 16 : 32), up(b) = b rounded up to 256, sort(m, g) as for
 * emd_raster_det_workspace_size:
 *     bytes = up(16 n C) + sort(4 n, g) + up(64) + 3 up(4 n) + up(8 * 16 * 2 ceil(n / EMD_SEG_CHUNK)) + 256
 *             the [4 n][C] rows, the sort and sum of 4 n slots, the count words, the time column with its keys and slots, its chunk sums
 * The size does not depend on the resolutions: the largest plane of the call decides the number of sort passes only. */
#define EMD_HEX_FLAG_DETERMINISTIC 1u
int emd_hexplane_det_workspace_size(const EmdHexArgs* args, size_t* bytes);                 /* host-only: reads num_points and channels */
/* Byte offsets inside det_ws for plane `plane` = 1 + 6 s + p (the coding of det_keep_plane), for tests and profiles: out[0] the [4 N][C] rows
 * out[1] / out[2] the key and slot buffers that hold the SORTED lists after that plane's number of sort passes  out[3] the [N] time column
 * out[4] the raw keys  out[5] the count words (uint32; [0] = slots the sort kept = 4 N)  out[6] = that number of passes (a value, not an offset)
 * out[7] = the total, as emd_hexplane_det_workspace_size reports it */
int emd_hexplane_det_workspace_offsets(const EmdHexArgs* args, int32_t plane, size_t out[8]);

/* Sort keys of the visiting orders the aggregating backward is handed (EmdHexArgs.order, EmdHexGrads.order2d): in ONE launch, per point, the
 * 30-bit Z-order key of its box-normalised position (10 bits per axis) -> keys[0 .. N) and the 24-bit HILBERT keys of its (x, y), (x, z),
 * (y, z) coordinates (12 bits per axis) -> keys[N .. 4 N).  Runs of consecutive points of the sorted keys are compact in 3-D / in that
 * plane; a Hilbert curve has no jumps, so a run of the per-plane pass stays inside its LDS window (a Z-order run leaves it with 7 % of its
 * taps at resolution 512).  aabb: six floats, the two corners of the box in either order (HexPlaneField.aabb); coordinates are clamped
 * into the box, NaN goes to cell 0.  [host side: emd_amd/hexplane.py VisitingOrders.build; no reference counterpart -- the reference's
 * grid_sample backward scatters in the order the points come] */
int emd_hexplane_order_keys(const float* pts, const float* aabb, int64_t num_points, int32_t* keys, void* hip_stream);

/* ---- embedding ops in front of the deformation MLPs (rows a3, a12, a15) ---------------------
 * emd_temporal_embed_*: one row of the coarse-to-fine temporal embedding -- each of the num_tables [rows, dim] tables resized
 *   to k rows (bilinear, align_corners) and sampled at time t[0] (bilinear, align_corners, reflection padding) -> out
 *   [num_tables, dim].  Replaces
 *   Deformation.get_temporal_embed (S3Gaussian/scene/deformation.py:208-221) and RigidNodes.get_temporal_embed
 *   (OmniRe/models/nodes/rigid.py:150-164).  t is a DEVICE scalar (no host sync).  The backward ACCUMULATES into dL_dweight
 *   [rows, dim] and dL_dt [1] (either may be NULL); the caller zeroes them.
 * emd_deform_input_*: the input matrix of OmniRe's ConditionalDeformNetwork (models/modules.py:411-457 with get_embedder
 *   :318-366, fed by DeformableNodes.get_deformation, models/nodes/deformable.py:35-47): row n =
 *   [x, sin(x 2^0), cos(x 2^0), ..., t, sin(t 2^0), ..., embed[id(n)]] with x = means[n] / inst_size[id(n)][2] * 2.
 *   The backward ACCUMULATES columns [col0, col0 + embed_dim) of dL_din into dL_dembed [A, embed_dim] (positions and the time
 *   are detached in the reference). */
int emd_temporal_embed_forward(const float* weight, int num_tables, int rows, int dim, int k, const float* t, float* out,
                               void* hip_stream);
int emd_temporal_embed_backward(const float* weight, int num_tables, int rows, int dim, int k, const float* t, const float* dL_dout,
                                float* dL_dweight, float* dL_dt, void* hip_stream);
/* The same gradients without atomics (a compatible extension of ABI 30), in gather form: one lane per column of the at most
 * four table rows a sample touches adds ITS contributions in the default kernel's issue order -- column j ascending, then the resized row r = 0, 1,
 * then (ha, x0), (hb, x0), (ha, x1), (hb, x1) --, each product formed as the default kernel forms it, in double precision from 0.0 with one
 * rounding, and WRITES the result to dL_dweight (the caller zeroes it, as for the default entry: rows no sample touches keep the zeros).  dL_dt: the
 * fixed xor tree of each table, the tables then added in ascending order by one thread onto the caller's value.  `dt_partials`: num_tables floats,
 * device, never cleared; needed when dL_dt is given and num_tables > 1 (EMD_ERR_WORKSPACE when missing). */
int emd_temporal_embed_backward_det(const float* weight, int num_tables, int rows, int dim, int k, const float* t, const float* dL_dout,
                                    float* dL_dweight, float* dL_dt, float* dt_partials, void* hip_stream);

/* Learned per-actor track offsets, all actors and both levels in one launch each way
 * (embedding_track_trans_offset / embedding_track_rot_offset / query_coarse_to_fine / get_temporal_embed,
 * OmniRe/models/nodes/rigid.py:150-246): see the block comment in csrc/embed.hip.  head_w[h] is [rows_h, dim + embed_dim]
 * row-major, head_b[h] is [rows_h], h = 0 track_trans_c (3 rows), 1 track_trans_f (3), 2 track_rot_c (1), 3 track_rot_f (1). */
typedef struct EmdTrackArgs {
    int32_t num_actors, rows, dim, embed_dim;    /* temporal tables [A, rows, dim]; dim + embed_dim <= 64 */
    int32_t k_coarse, k_fine, num_points, reserved;
    float t;                                     /* normalised frame (frame - start) / (end - start), rigid.py:204,241 */
    const float* t_dev;                          /* optional DEVICE copy of t (overrides it): hipGraph replay with a new frame */
    const int32_t* k_fine_dev;                   /* optional DEVICE copy of k_fine (overrides it): the coarse-to-fine row count follows the
                                                    training step (rigid.py:194-201), which a replayed graph reads from the device (ABI 18) */
    const float* weight;                         /* [A, rows, dim] */
    const float* embeddings;                     /* [num_points, embed_dim] of the actor Gaussians */
    const int32_t* point_ids;                    /* [num_points] actor of every point (-1: none) */
    const float* count;                          /* [A] points per actor, as floats */
    const int32_t* segment_start;                /* [A+1] or NULL: point_ids are sorted and actor a owns points [start[a], start[a+1]) -- the
                                                    sums are then formed without atomics and emb_sum need not be zero-filled */
    const float* head_w[4];
    const float* head_b[4];
    float* emb_sum;                              /* [A, embed_dim] scratch: per-actor embedding sums; ZERO-FILLED by the caller before forward, kept for backward */
    float* trans;                                /* out [A,3] */
    float* rot;                                  /* out [A,4] (w,x,y,z) */
} EmdTrackArgs;

typedef struct EmdTrackGrads {
    const float* g_trans;                        /* [A,3] */
    const float* g_rot;                          /* [A,4] */
    float* d_weight;                             /* [A, rows, dim]; accumulated into: ZERO-FILLED by the caller, like d_head_w / d_head_b */
    float* d_embeddings;                         /* [num_points, embed_dim] or NULL */
    float* d_head_w[4];
    float* d_head_b[4];
    float* d_mean;                               /* [A, embed_dim] scratch */
} EmdTrackGrads;

int emd_track_heads_forward(const EmdTrackArgs* args, void* hip_stream);
int emd_track_heads_backward(const EmdTrackArgs* args, const EmdTrackGrads* grads, void* hip_stream);

/* The per-actor chain of a training step in ONE launch each way (ABI 18): embedding sums -> track heads -> pose row
 * (= emd_track_heads_forward + emd_actor_pose_forward: RigidNodes.transform_means / transform_quats with the learned offsets,
 * OmniRe/models/nodes/rigid.py:150-246,499-566), one 1024-thread workgroup per actor.  Needs track.segment_start (an actor's
 * points contiguous, as the reference stores them) and embed_dim <= 8.  track.trans / track.rot are optional outputs here.
 * The backward WRITES d_q_all / d_t_all (the dense [F, A, .] clip gradients, zero outside the frame), d_weight and d_embeddings in
 * full and ADDS the head gradients into d_head_w / d_head_b, which must be views of the `head_acc` buffer the FORWARD call of the
 * same step was given (it clears those head_acc_floats floats): the caller zero-fills nothing.  A second backward through one
 * forward must clear head_acc itself. */
typedef struct EmdTrackedPoseArgs {
    EmdTrackArgs track;
    const float* q_all;                          /* [F, A, 4] raw per-frame pose quaternions (instances_quats) */
    const float* t_all;                          /* [F, A, 3] (instances_trans) */
    const uint8_t* valid_all;                    /* [F, A] bytes or NULL (instances_fv) */
    int32_t num_frames, frame;                   /* frame: row of the tables, unless frame_dev is given */
    const int32_t* frame_dev;                    /* optional DEVICE frame index (hipGraph replay) */
    float* pose;                                 /* out [A, EMD_ACTOR_STRIDE] */
    float* head_acc;                             /* forward: cleared (may be NULL when no backward will follow) */
    int32_t head_acc_floats, reserved;
} EmdTrackedPoseArgs;

typedef struct EmdTrackedPoseGrads {
    const float* g_pose;                         /* [A, EMD_ACTOR_STRIDE] */
    float* d_q_all;                              /* [F, A, 4] */
    float* d_t_all;                              /* [F, A, 3] */
    float* d_weight;                             /* [A, rows, dim] */
    float* d_embeddings;                         /* [num_points, embed_dim] or NULL */
    float* d_head_w[4];                          /* accumulated into: views of the forward's head_acc */
    float* d_head_b[4];
} EmdTrackedPoseGrads;

int emd_tracked_pose_forward(const EmdTrackedPoseArgs* args, void* hip_stream);
int emd_tracked_pose_backward(const EmdTrackedPoseArgs* args, const EmdTrackedPoseGrads* grads, void* hip_stream);

typedef struct EmdDeformInArgs {
    int32_t num_points, num_freqs_x, num_freqs_t, embed_dim;
    int32_t ld, reserved;                        /* row stride of out in floats (>= emd_deform_input_width) */
    const float* means;                          /* [N,3] local means */
    const int32_t* point_ids;                    /* [N] actor of each point; NULL: row n of inst_size / inst_embed belongs to point n */
    const float* inst_size;                      /* [A,3] actor box sizes (height = [.,2]); NULL: means are used as given */
    const float* inst_embed;                     /* [A, embed_dim] */
    const float* t;                              /* device scalar: normalised time of the frame */
    float* out;                                  /* [N, ld] */
} EmdDeformInArgs;

int emd_deform_input_width(int num_freqs_x, int num_freqs_t, int embed_dim);
int emd_deform_input_forward(const EmdDeformInArgs* args, void* hip_stream);
int emd_deform_input_backward(int num_points, int embed_dim, int ld, int col0, const int32_t* point_ids, const float* dL_din,
                              float* dL_dembed, void* hip_stream);

/* ---- The actor chain and the encoder-input gradient without float atomics (csrc/track_det.hip).  Opt-in entry points of their
 * own: a compatible extension (no struct changed, EMD_ABI_VERSION kept); the default entries and their kernels are untouched.  Nothing of what they
 * compute depends on workgroup order, the stream, other work on the device, or eager execution against hipGraph replay.
 *
 * Workspace `ws` of every entry below: caller-owned, device, 256-byte aligned, never cleared; missing, misaligned or shorter than
 * emd_track_det_workspace_size reports for the call is EMD_ERR_WORKSPACE, decided before anything is launched.  Layout for (num_actors A, head_width w,
 * num_points n, row_width g), up(b) = b rounded up to 256, sort(m, g) as for emd_raster_det_workspace_size:
 *     bytes = up(4 A pitch) + up(4 * 128 A) + sort(n, min(g, 32)) + up(64) + 256,   pitch = 8 w + 8 rounded up to 16 floats
 *             the slab [A][pitch], the per-lane dL/dh rows [A][2][64], the sort by actor with the chunk sums, the count words
 * -- the first two terms only when w > 0 (the chain's backward), the sort only when g > 0 and n > 0 (the row sum).  emd_track_det_workspace_size is
 * host-only and returns 0 for sizes outside the limits (w <= 64, g <= 64, n <= 2^31 - 1 - 2048).  emd_track_det_workspace_offsets: out[0] byte offset of
 * the slab, [1] its pitch IN FLOATS, [2] byte offset of the dL/dh rows, [3] the raw keys (actor of every point, 0xFFFFFFFF = none), [4] the sorted keys
 * and [5] the sorted point indices (the ping-pong pair that holds the result for this A), [6] the count words (uint32 [0] = points the sort kept),
 * out[7] = the total.
 *
 * emd_actor_row_sum_det: out[a * out_pitch + f], f < width, = the sum of rows[i * row_pitch + f] over the points i with ids[i] == a in ASCENDING i with
 *   the association of emd_segmented_row_sum (chunks of EMD_SEG_CHUNK = 512, fp64 from 0.0, one rounding).  An actor without a point gets +0.0 (written
 *   here: `out` need not be initialised); an id outside [0, num_actors) contributes nothing.  1 <= width <= 64 (columns in bands of at most 32 over one
 *   sorted list), row_pitch, out_pitch >= width; EMD_ERR_INVALID otherwise.  segment_start ([num_actors + 1], start[0] = 0, start[A] = n; or NULL): the
 *   ids are sorted by actor and the sort is skipped -- the association depends on run length and position alone, so the bits are the same.  n == 0 or
 *   num_actors == 0 launches nothing and needs no workspace.  ws: (num_actors, 0, n, width).
 * emd_track_heads_forward_det: emd_track_heads_forward with the embedding sums formed by emd_actor_row_sum_det when segment_start is NULL or
 *   embed_dim > 8 (emb_sum need not be zero-filled; ws: (A, 0, num_points, embed_dim)); otherwise the default forward, which has no atomics, as it is
 *   (ws may be NULL).
 * emd_track_heads_backward_det / emd_tracked_pose_backward_det: emd_track_heads_backward / emd_tracked_pose_backward with every refusal of theirs;
 *   ws: (A, dim + embed_dim, 0, 0).  Nothing arrives zero-filled and the forward clears nothing (EmdTrackedPoseArgs.head_acc = NULL there):
 *   - head gradients: actor a STORES its share of the eight head tensors to slab[a] -- the tensors back to back as head_acc has them, w_tc b_tc w_tf
 *     b_tf w_rc b_rc w_rf b_rf, 8 w + 8 floats, each product formed as the default forms it, +0.0 where the default skips the add of a zero gradient --
 *     and one launch adds the slots per element in ascending actor index in fp64 from 0.0, rounds once and writes all 8 w + 8 destination elements;
 *   - d_weight, in gather form: the at most eight touched rows of an actor's table are slots q = 4 level + 2 r + (0: ha, 1: hb); the lane of (q, c)
 *     owns element (row[q], c) when no earlier slot names the same row and adds its contributions in the default's issue order -- column j ascending,
 *     coarse before fine, r = 0, 1, then (ha, x0), (hb, x0), (ha, x1), (hb, x1) --, each product g * wx * wy * l formed left to right in fp32 without
 *     contraction, in fp64 from 0.0 with one rounding; every other element of [A, rows, dim] is written +0.0;
 *   - the per-lane dL/dh_c and dL/dh_f of every actor are left in the workspace ([A][2][64]);
 *   - d_q_all / d_t_all / d_mean / d_embeddings are per actor or per point and keep the default's arithmetic. */
size_t emd_track_det_workspace_size(int32_t num_actors, int32_t head_width, int64_t num_points, int32_t row_width);
int emd_track_det_workspace_offsets(int32_t num_actors, int32_t head_width, int64_t num_points, int32_t row_width, size_t out[8]);
int emd_actor_row_sum_det(int32_t n, int32_t width, const float* rows, int32_t row_pitch, const int32_t* ids, int32_t num_actors,
                          const int32_t* segment_start, float* out, int32_t out_pitch, void* ws, size_t ws_bytes, void* hip_stream);
int emd_track_heads_forward_det(const EmdTrackArgs* args, void* ws, size_t ws_bytes, void* hip_stream);
int emd_track_heads_backward_det(const EmdTrackArgs* args, const EmdTrackGrads* grads, void* ws, size_t ws_bytes, void* hip_stream);
int emd_tracked_pose_backward_det(const EmdTrackedPoseArgs* args, const EmdTrackedPoseGrads* grads, void* ws, size_t ws_bytes, void* hip_stream);

/* ---- The width-64 MLPs of the EMD deformation network as fused fp32-MFMA kernels -------------------
 * Deformation.feature_out (defor_depth = 1) + the pos / scales / rotations / opacity / shs heads + dino_head of
 * S3Gaussian/scene/deformation.py:100-185,254-337: see the block comment of csrc/mlp.hip.  One trunk call and one branch call per
 * head replace ~12 GEMMs and ~30 element-wise launches per level and direction; every intermediate stays in registers.
 *   trunk   h = b + w[:, col_a : col_a + ka] xa + w[:, col_b : col_b + kb] xb      (ka a multiple of 4 up to 128, kb <= 8; b = the layer's bias +
 *           the contribution of the temporal-embedding row, which is the same for every Gaussian)
 *   branch  out = w_out act(... act(w_hidden[0] in + b_hidden[0]) ...) + b_out, `depth` hidden layers of width 64 with ReLU,
 *           in = relu(h) when relu_input (the deformation heads: nn.Sequential(ReLU, Linear, ReLU, Linear)) else h (dino_head)
 * Backward: each branch writes ITS contribution to dL/dh into its own [N,64] buffer (the ReLU mask of relu_input applied) and
 * ACCUMULATES its weight / bias gradients with float atomics (the caller zero-fills them); the trunk sums the contributions,
 * writes dL/dxa, dL/dxb and accumulates the xa / xb column blocks of d_w and d_b.  All matrices row-major fp32; xa, h, g_h, d_xa
 * 16-byte aligned. */
#define EMD_MLP_MAX_BRANCHES 6
typedef struct EmdMlpTrunk {
    int32_t num_points, ka, kb, ld_w;            /* ld_w: row stride of w (the nn.Linear weight [64, ld_w]) */
    int32_t col_a, col_b, reserved0, reserved1;  /* first column of the xa / xb block inside w */
    const float* xa;                             /* [N, ka] or NULL */
    const float* xb;                             /* [N, kb] or NULL */
    const float* w;                              /* [64, ld_w] */
    const float* b;                              /* [64] effective bias */
    float* h;                                    /* [N, 64] pre-activation: written by the forward; the backward does not read it (may be NULL there, ABI 26) */
} EmdMlpTrunk;

typedef struct EmdMlpTrunkGrads {
    int32_t num_gh, reserved;
    const float* g_h[EMD_MLP_MAX_BRANCHES];      /* [N,64] each: summed */
    float* d_xa;                                 /* [N, ka] or NULL */
    float* d_xb;                                 /* [N, kb] or NULL */
    float* d_w;                                  /* [64, ld_w] accumulated (xa / xb column blocks only) or NULL */
    float* d_b;                                  /* [64] accumulated or NULL */
} EmdMlpTrunkGrads;

typedef struct EmdMlpBranch {
    int32_t num_points, depth, relu_input, out_dim;   /* depth 1 or 2; out_dim 1..64 */
    const float* h;                              /* [N,64] */
    const float* w_hidden[2];                    /* [64,64] each */
    const float* b_hidden[2];                    /* [64] */
    const float* w_out;                          /* [out_dim,64] */
    const float* b_out;                          /* [out_dim] */
    float* out;                                  /* [N,out_dim] (forward) */
    float* l1_sum;                               /* optional (ABI 20), [1], ZEROED BY THE CALLER: the forward adds mean |out| to it -- the L1 regulariser
                                                    of a residual head (S3Gaussian/train.py:238-310) formed while the outputs are stored */
    /* optional (ABI 26), depth 1 only: a level WITHOUT HexPlane features (`no_fine_hexplane_features`, the reference's run script: the trunk's
     * input is the per-Gaussian embedding alone, S3Gaussian/scene/deformation.py:256-296).  h = b_in + w_in[:, col_in : col_in + kb_in] xb is then
     * eight fp32 MFMAs per 32 rows: with `xb` set the head forms h itself, in the trunk kernel's operation order (same bits), and `h` may be NULL --
     * no [N,64] tensor is written by a trunk launch and read back by every head, forward and backward. */
    const float* xb;                             /* [N,kb_in] */
    const float* w_in;                           /* the trunk's weight [64, ld_w_in] */
    const float* b_in;                           /* [64]: its bias plus whatever is constant over the Gaussians */
    int32_t kb_in, ld_w_in, col_in, reserved;    /* kb_in 1..8 */
} EmdMlpBranch;

typedef struct EmdMlpBranchGrads {
    const float* g_out;                          /* [N,out_dim] */
    float* g_h;                                  /* [N,64] out */
    float* d_w_hidden[2];                        /* accumulated; any may be NULL */
    float* d_b_hidden[2];
    float* d_w_out;
    float* d_b_out;
    /* optional (ABI 20): the gradient of l1_sum's mean |out|, folded into g_out while it is loaded: g_out[i] + sign(out[i]) l1_grad[0] / (N out_dim).
     * `out` is the forward's output tensor; g_out may then be NULL (no other gradient reaches the head). */
    const float* l1_grad;                        /* [1], device */
    const float* out;                            /* [N,out_dim] */
    /* optional (ABI 20): g_h = g_h_in + this head's contribution (g_h_in may be g_h itself: every element is read and written by the same
     * lane).  Chaining the heads of a level through ONE buffer leaves the trunk's backward a single [N,64] tensor to read instead of one
     * per head.  Depth 1 only (the two-hidden-layer kernel has no registers for the extra tile: EMD_ERR_INVALID). */
    const float* g_h_in;                         /* [N,64] or NULL */
} EmdMlpBranchGrads;

int emd_mlp_trunk_forward(const EmdMlpTrunk* args, void* hip_stream);
int emd_mlp_trunk_backward(const EmdMlpTrunk* args, const EmdMlpTrunkGrads* grads, void* hip_stream);
int emd_mlp_branch_forward(const EmdMlpBranch* args, void* hip_stream);
int emd_mlp_branch_backward(const EmdMlpBranch* args, const EmdMlpBranchGrads* grads, void* hip_stream);

/* ---- Deterministic forms of the MLP kernels: no float atomics (a compatible extension of ABI 30) --------------
 * The default kernels above add one total per workgroup onto every weight / bias gradient element (and onto l1_sum) with float atomics: the
 * order in which the up to 512 workgroups of a launch reach an address is the only scheduling-dependent step.  The forms below run the SAME
 * kernel bodies up to and including the workgroup's sum and then STORE the total to slot blockIdx.x of a slab [G][pitch] per tensor, with the
 * default flush's bounds: every workgroup writes every element of its slot, zeros included, so the slab is caller-owned, 256-byte aligned and
 * NEVER cleared.  emd_mlp_det_reduce then adds, per destination element, the G slots in ascending workgroup order in double precision from 0.0,
 * multiplies by the job's scale (still in double precision), rounds once to float and WRITES the result: the destination need not be cleared,
 * and elements the default kernels never add to (the temporal columns of the trunk's d_w) are not written.  Every other output (out, g_h, d_xa,
 * d_xb) has the default call's bits.  (A bias partial lives in both lane halves of wave 0, which the atomic form adds onto one address: the slab
 * holds lower half + upper half, added in that order.)
 *   G = the grid of the kernel that serves the call: ceil(ceil(N / 32) / 4) workgroups, at most 256 per_cu (per_cu = 2 for the forward of a
 *   one-hidden-layer head of at most 32 outputs and for the trunk backward with ka = 0 outside the embedding kernel, else 1).
 *   tensors of a slab, in this order, `pitch` floats per slot, element (o, i) of the [rows, cols] gradient block at o cols + i:
 *     EMD_MLP_DET_BRANCH_BWD  0 d_w_hidden[0] 4096 | 1 d_b_hidden[0] 64 | 2 d_w_hidden[1] 4096 | 3 d_b_hidden[1] 64 (pitch 0 for depth 1) |
 *                             4 d_w_out 64 out_dim | 5 d_b_out out_dim
 *     EMD_MLP_DET_TRUNK_BWD   0 d_w[:, col_a : col_a + ka] 64 ka | 1 d_w[:, col_b : col_b + kb] 64 kb | 2 d_b 64
 *     EMD_MLP_DET_BRANCH_FWD  0 the workgroup's share of sum |out|, 1 float (scale of the reduction: 1 / (N out_dim))
 *   offset[t] (bytes, multiples of 256) = the sum of the earlier tensors' 4 G pitch bytes, each rounded up to 256; bytes = the end of the last.
 * emd_mlp_det_slab_bytes is host-only: it fills *layout (may be NULL) and returns `bytes`; 0 for num_points == 0 or arguments the entry points
 * refuse.  `grads` is read by EMD_MLP_DET_TRUNK_BWD alone (the alignment of d_xb takes part in the choice of the kernel) and may be NULL.
 * The entry points apply every refusal of the default ones; a missing, unaligned (256 B) or short slab is EMD_ERR_WORKSPACE, decided before
 * anything is launched; num_points == 0 launches nothing and needs no slab.  The forward form needs l1_sum (it is what the call is for). */
#define EMD_MLP_DET_MAX_TENSORS 6
#define EMD_MLP_DET_MAX_JOBS 64
enum { EMD_MLP_DET_BRANCH_BWD = 0, EMD_MLP_DET_TRUNK_BWD = 1, EMD_MLP_DET_BRANCH_FWD = 2 };
typedef struct EmdMlpDetLayout {
    int32_t groups, num_tensors;                 /* G; 6 / 3 / 1 */
    int32_t pitch[EMD_MLP_DET_MAX_TENSORS];      /* floats per slot (0: the call has no such tensor) */
    size_t offset[EMD_MLP_DET_MAX_TENSORS];      /* bytes from the slab's start */
    size_t bytes;
} EmdMlpDetLayout;
typedef struct EmdMlpDetJob {
    const float* slab;                           /* [groups][pitch], pitch >= rows cols */
    float* dst;                                  /* element (o, i) -> dst[o ld + col0 + i] = (float)(scale * sum over the slots, ascending) */
    int32_t groups, pitch, rows, cols, ld, col0;
    double scale;
} EmdMlpDetJob;
size_t emd_mlp_det_slab_bytes(int kind, const void* args, const void* grads, EmdMlpDetLayout* layout);
int emd_mlp_branch_forward_det(const EmdMlpBranch* args, void* l1_slab, size_t slab_bytes, void* hip_stream);
int emd_mlp_branch_backward_det(const EmdMlpBranch* args, const EmdMlpBranchGrads* grads, void* slabs, size_t slab_bytes, void* hip_stream);
int emd_mlp_trunk_backward_det(const EmdMlpTrunk* args, const EmdMlpTrunkGrads* grads, void* slabs, size_t slab_bytes, void* hip_stream);
/* `jobs`: a HOST array of 1..EMD_MLP_DET_MAX_JOBS jobs (passed to the one launch by value: nothing is read from it after the call returns).
 * groups >= 1, pitch >= rows cols, rows, cols >= 1, ld >= col0 + cols, non-NULL pointers; EMD_ERR_INVALID otherwise. */
int emd_mlp_det_reduce(const EmdMlpDetJob* jobs, int num_jobs, void* hip_stream);

/* ---- emd_deform_mlp_*: OmniRe's ConditionalDeformNetwork (models/modules.py:411-457) from its encoded input, on fp32 MFMA (csrc/deform_mlp.hip) ----
 * A compatible extension (no struct changed, EMD_ABI_VERSION kept).  No BLAS, no float atomics, no second mode: every output and every gradient is a
 * fixed function of the call's inputs (bit-identical from run to run, on any stream, under graph replay).  All products are exact fp32 MFMA fmaf chains.
 * Network (N rows, D = depth layers of width W, C = in_dim = the row width of emd_deform_input_forward, E = embed_dim = its last columns):
 *   h_0 = relu(b_0 + x W_0^T)                                        W_0 [W][C]
 *   h_i = relu(b_i + h_{i-1} W_i^T)                                  W_i [W][W]
 *   h_i = relu(b_i + x W_i[:, :C]^T + h_{i-1} W_i[:, C:]^T)          i = skip + 1, W_i [W][C + W]: read in place, no concat (skip = -1: no such layer)
 *   out[k] = b_head[k] + h_{D-1} w_head[k]^T                         k = 0 warp [N][3], 1 rotation [N][4], 2 scaling [N][3]; w_head[k] NULL: head absent
 * Summation order: an accumulator starts at the bias, takes the x block before the h block, and inside a block the input columns in ascending blocks of
 * 32; inside a block of 32 the MFMA pairs columns (8 a + j, 8 a + 4 + j), a = 0..3, j = 0..3, in that order.  It does not depend on N or on the grid.
 * Backward (G_i = dL/dh_i where h_i > 0, else 0):
 *   dL/dh_{D-1}[n][c] = fmaf chain from 0 over g_out[0][n][0..2], g_out[1][n][0..3], g_out[2][n][0..2] (absent heads skipped) times w_head[.][c]
 *   dL/dh_{i-1} = G_i W_i (the h block of the skip layer), dL/dx[:, C-E : C] = G_i W_i[:, C-E : C] for i = skip + 1 and i = 0: the accumulator starts at
 *   0 and sums over the W output features in the order above.  Positions and time are detached in the reference, so only these E columns of d_x are
 *   written (element (n, j) at d_x[n ld_dx + C - E + j]); with a skip layer the skip layer's launch stores its sum s and layer 0's launch, which runs
 *   later, stores s + (its own sum), in that order.
 *   d_w_i = G_i^T [input], d_b_i = sum_n G_i; d_w_head / d_b_head the same from g_out: the rows are cut into `groups` static groups of `group_rows`
 *   (EmdDeformMlpLayout: a function of N and num_cus alone), a workgroup sums its group's rows in ascending steps of 32 (inside a step the MFMA pairs row s
 *   with row 16 + s, s = 0..15; a bias partial is rows 0..15 + rows 16..31 per step) and stores the total to slot `group` of the slab; the slots are then
 *   added in ascending order in double precision from 0.0 and rounded once.  Every slot element is written: the slab is never cleared, and its one region
 *   serves layer after layer (the launches are stream-ordered).
 * Slab: groups = ceil(N / group_rows), group_rows = max(EMD_DEFORM_MLP_MIN_GROUP_ROWS, ceil(N / max(1, num_cus / 2))) rounded up to 32;
 *   [groups][pitch_w = W max(W, C)] floats at offset_w = 0, [groups][pitch_b = W] floats at offset_b, each rounded up to 256 bytes.
 * emd_deform_mlp_workspace is host-only.  Every buffer is caller-owned; the library allocates nothing.  Refused before anything is launched:
 *   EMD_ERR_INVALID  width not a multiple of 32 or > 256; depth < 2 or > EMD_DEFORM_MLP_MAX_LAYERS; skip == depth - 1 (the heads would see the concat)
 *                    or outside -1 .. depth - 2; in_dim > 256; embed_dim > min(32, in_dim); ld_x < in_dim; num_cus < 1; a NULL required pointer;
 *                    h[i] / g_h[k] not 16-byte aligned;
 *   EMD_ERR_WORKSPACE  a missing slab, one not 256-byte aligned or shorter than the layout's `bytes`.
 * num_points == 0 launches nothing.  The forward writes h[0 .. D-1] (the saved post-ReLU activations the backward reads) and out[k]; the backward
 * does not read out[k] (it may be NULL there). */
#define EMD_DEFORM_MLP_MAX_LAYERS 16
#define EMD_DEFORM_MLP_MIN_GROUP_ROWS 256
typedef struct EmdDeformMlpArgs {
    int32_t num_points, depth, width, in_dim, embed_dim, skip;
    int32_t ld_x, num_cus;                       /* row stride of x in floats; compute units of the device (the row groups of the backward) */
    const float* x;                              /* [N][ld_x] encoded input */
    const float* w[EMD_DEFORM_MLP_MAX_LAYERS];
    const float* b[EMD_DEFORM_MLP_MAX_LAYERS];
    float* h[EMD_DEFORM_MLP_MAX_LAYERS];         /* [N][W] each, 16-byte aligned */
    const float* w_head[3];
    const float* b_head[3];
    float* out[3];
} EmdDeformMlpArgs;
typedef struct EmdDeformMlpGrads {
    const float* g_out[3];                       /* dL/dout[k] of every present head */
    float* d_w[EMD_DEFORM_MLP_MAX_LAYERS];
    float* d_b[EMD_DEFORM_MLP_MAX_LAYERS];
    float* d_w_head[3];
    float* d_b_head[3];
    float* d_x;                                  /* [N][ld_dx] or NULL; columns C-E .. C-1 are written */
    int32_t ld_dx, reserved;
    float* g_h[2];                               /* scratch: two distinct [N][W] buffers, 16-byte aligned */
    void* slab;
    size_t slab_bytes;
} EmdDeformMlpGrads;
typedef struct EmdDeformMlpLayout {
    int32_t groups, group_rows, pitch_w, pitch_b;
    size_t offset_w, offset_b, bytes;
} EmdDeformMlpLayout;
int emd_deform_mlp_workspace(int num_points, int width, int in_dim, int num_cus, EmdDeformMlpLayout* layout);
int emd_deform_mlp_forward(const EmdDeformMlpArgs* args, void* hip_stream);
int emd_deform_mlp_backward(const EmdDeformMlpArgs* args, const EmdDeformMlpGrads* grads, void* hip_stream);

/* ---- Adaptive density control on the device ----------------------------------------------------
 * densify = densify_and_clone + densify_and_split, prune = prune / prune_points of S3Gaussian/scene/gaussian_model.py:441-603,
 * 683-701 (OmniRe: models/gaussians/vanilla.py:206-376), rewriting the SoA parameters, both Adam moments and the statistics in
 * one gather launch -- see the block comment of csrc/densify.hip.  Call sequence of one event:
 *   emd_densify_decide  -> code[N], block_counts[3][ceil(N / 256)] (per 256-point block: survivors, clones, splits)
 *   emd_densify_scan    -> the counts become exclusive block offsets; totals[3]: num_out = keep + clone + 2 split is the event's one host read
 *   emd_densify_index   -> src[num_out], kind[num_out] (0 survivor, 1 clone, 2 / 3 split sample replica 0 / 1), in the
 *                          reference's output order: survivors, clones, replica 0, replica 1
 *   emd_densify_gather  -> every output tensor
 * Thresholds are the host's products (size_threshold = percent_dense * scene_extent, 0.1 * scene_extent) formed in double and rounded to float
 * once, as torch rounds a Python scalar: the device multiplies nothing (a product of two rounded floats differs from it by an ulp for about
 * a quarter of all extents, and a Gaussian whose max exp(scale) sits between the two would be cloned where the reference splits it). */
enum { EMD_DENSIFY_MODE_DENSIFY = 0, EMD_DENSIFY_MODE_PRUNE = 1,
       EMD_DENSIFY_MODE_REFINE = 2   /* OmniRe's per-class refinement (VanillaGaussians.refinement_after, models/gaussians/vanilla.py:206-297): split (the original
                                        STAYS, its log-scale reduced in place), duplicate and cull as ONE event -- see EmdRefineArgs below */ };
enum {
    EMD_DENSIFY_ROLE_COPY = 0,     /* parameter copied row for row (features, opacity, rotation, embedding, deformation table ...) */
    EMD_DENSIFY_ROLE_XYZ = 1,      /* means: split samples get R(q) (exp(scaling) * n) + xyz, n ~ N(0, 1)   gaussian_model.py:541-545 */
    EMD_DENSIFY_ROLE_SCALING = 2,  /* log-scales: split samples get log(exp(s) / (0.8 * 2))                  gaussian_model.py:546 */
    EMD_DENSIFY_ROLE_STATE = 3,    /* Adam moment: survivors keep theirs, new rows start at zero             gaussian_model.py:480-500 */
    EMD_DENSIFY_ROLE_ZERO = 4      /* statistics: reset to zero by a densification (gaussian_model.py:526-530), carried by a prune */
};

typedef struct EmdDensifyArgs {
    int32_t num_points, mode;
    const float* scaling;          /* [N,3] log-scales */
    const float* opacity;          /* [N] logits (prune) */
    const float* grad_accum;       /* [N] xyz_gradient_accum (densify) */
    const float* denom;            /* [N] (densify) */
    const float* max_radii2D;      /* [N] (prune with max_screen_size > 0) */
    const uint8_t* extra_drop;     /* [N] or NULL: additional rows to drop in prune mode (prune_points(mask) with a caller's mask) */
    float grad_threshold;                                   /* densify */
    float size_threshold;                                   /* densify: percent_dense * scene_extent (clone where max exp(scale) <= it, split above);
                                                               prune: 0.1 * scene_extent (drop where max exp(scale) > it) */
    float min_opacity, max_screen_size;                     /* prune; max_screen_size <= 0: the size tests are off */
} EmdDensifyArgs;

typedef struct EmdDensifyTensor {
    const float* src;              /* [N, width] */
    float* dst;                    /* [num_out, width] */
    int32_t width, role;
} EmdDensifyTensor;

#define EMD_DENSIFY_MAX_TENSORS 40
typedef struct EmdDensifyGather {
    int32_t num_out, num_tensors, mode, num_split;
    const int32_t* src;            /* [num_out] */
    const int32_t* kind;           /* [num_out] */
    const float* scaling;          /* [N,3] source log-scales  (split) */
    const float* rotation;         /* [N,4] source quaternions (split) */
    uint64_t seed;                 /* Philox key of the split samples: counter = (source Gaussian index, replica) -- the same samples on
                                      every rank of a data-parallel job without communication */
    const float* samples;          /* [2, num_split, 3] standard normals to use INSTEAD of Philox (tests: the reference's recorded draw) or NULL */
    const int32_t* split_rank;     /* [num_out] rank of a split row inside its replica (emd_densify_split_rank); needed with `samples` */
    EmdDensifyTensor tensors[EMD_DENSIFY_MAX_TENSORS];
} EmdDensifyGather;

/* ---- OmniRe refinement: VanillaGaussians.refinement_after = split_gaussians + dup_gaussians + cull_gaussians, models/gaussians/vanilla.py:206-376,
 * and dup_in_optim / remove_from_optim, models/gaussians/basics.py:198-242 -- fused into ONE decide -> scan -> index -> gather event.
 * Semantics restated from the reference (they differ from S3Gaussian's in every step):
 *   high   = xys_grad_norm / vis_counts > densify_grad_thresh                               (no NaN -> 0 step: NaN compares false)
 *   split  = (max exp(scale) > size_thresh  [or max_2Dsize > split_screen while step < stop_screen_size_at]) and high
 *            -> n_split_samples new rows  R(q^)(exp(scale) * n) + mean, n ~ N(0,1), scale log(exp(s) / 1.6); the ORIGINAL stays and takes the
 *               same reduced scale in place (vanilla.py:345)
 *   dup    = (max exp(scale) <= size_thresh) and high, evaluated AFTER the in-place reduction: a Gaussian just above the threshold is split
 *            AND duplicated (its duplicate carries the reduced scale)                        (vanilla.py:240-254)
 *   cull   = on every row of the grown arrays: sigmoid(opacity) < cull_alpha, or -- past the first opacity reset -- max exp(scale) > cull_size,
 *            or (while step < stop_screen_size_at) max_2Dsize > cull_screen, new rows carrying max_2Dsize 0       (vanilla.py:299-326)
 *   output order: surviving originals, split samples replica 0, replica 1, ..., duplicates (vanilla.py:256-263); Adam moments of new rows zero.
 * Thresholds are the host's products (size_thresh = densify_size_thresh * scene_scale ...) rounded to float once, as torch rounds a Python scalar.
 * Sequence: emd_refine_decide -> code[N], per-block counts of four 0/1 columns (original kept, duplicate kept, samples kept, source is split) ->
 * emd_densify_scan (4 columns; one host read of the totals: num_out = keep + num_samples * samples + dup) -> emd_refine_index ->
 * emd_densify_gather with mode EMD_DENSIFY_MODE_REFINE. */
typedef struct EmdRefineArgs {
    int32_t num_points;
    int32_t do_densify;            /* split / duplicate this event (step < stop_split_at and past the opacity-reset guard, vanilla.py:213-216) */
    int32_t do_cull;               /* cull this event (vanilla.py:281) */
    int32_t use_split_screen;      /* step < stop_screen_size_at: the screen-size split test is on */
    int32_t cull_big;              /* step > reset_alpha_interval: the world-size (and screen-size) cull tests are on */
    int32_t use_cull_screen;       /* ... and step < stop_screen_size_at */
    const float* scaling;          /* [N,3] log-scales */
    const float* opacity;          /* [N] logits */
    const float* grad_norm;        /* [N] xys_grad_norm */
    const float* vis_counts;       /* [N] */
    const float* max_2Dsize;       /* [N] */
    float grad_threshold, size_threshold, split_screen, cull_alpha, cull_size, cull_screen;
} EmdRefineArgs;
int emd_refine_decide(const EmdRefineArgs* args, int32_t* code /*[N]*/, int32_t* block_counts /*[4, ceil(N / 256)]*/, void* hip_stream);
/* kind[j]: 0 original, 1 duplicate, 2 + r split sample of replica r; + 16 when the source row was split (its scale is reduced wherever it is
 * copied); split_rank[j]: rank of a sample's source among ALL split sources (the row of a caller-supplied normal draw [num_samples, n_split, 3]) */
int emd_refine_index(int32_t num_points, int32_t num_out, int32_t num_samples, const int32_t* code, const int32_t* block_offsets /*[4, ceil(N / 256)]*/,
                     const int32_t* totals /*[4]*/, int32_t* src, int32_t* kind, int32_t* split_rank, void* hip_stream);

/* OmniRe's running refinement statistics of one view (VanillaGaussians.after_train, models/gaussians/vanilla.py:163-191), one launch: where radii > 0
 * grad_norm += |xys_grad| (2 components, row stride `grad_stride` floats), vis_counts += 1, max_2Dsize = max(max_2Dsize, radii / last_size). */
int emd_after_train_stats(int32_t n, const int32_t* radii, const float* xys_grad, int32_t grad_stride, float* grad_norm, float* vis_counts,
                          float* max_2Dsize, float last_size, void* hip_stream);

int emd_densify_decide(const EmdDensifyArgs* args, int32_t* code /*[N]*/, int32_t* block_counts /*[3, ceil(N / 256)]*/, void* hip_stream);
/* exclusive prefix sums of the per-block counts over the blocks, in place, + totals[c] = sum of column c (device int32[num_columns]) */
int emd_densify_scan(int32_t num_points, int32_t num_columns, int32_t* block_counts, int32_t* totals, void* hip_stream);
int emd_densify_index(int32_t num_points, int32_t num_out, const int32_t* code, const int32_t* block_offsets /*[3, ceil(N / 256)]*/,
                      const int32_t* totals /*[3]*/, int32_t* src, int32_t* kind, void* hip_stream);
int emd_densify_split_rank(int32_t num_out, int32_t n_keep, int32_t n_clone, int32_t n_split, int32_t* rank, void* hip_stream);
int emd_densify_gather(const EmdDensifyGather* args, void* hip_stream);

/* ---- ABI 31 extension (new entry points and one struct only, so the number stays): refinement of the OmniRe ACTOR classes ------------------
 * RigidNodes / DeformableNodes.refinement_after (models/nodes/rigid.py:278-465): the event of EmdRefineArgs above on rows that carry an actor id,
 * plus `cull_out_of_bound`: a row is culled when it leaves its actor's box.  The reference tests every row of the GROWN arrays, so a split
 * sample at its new, sampled position: each replica lives or dies on its own (emd_refine_decide keeps one flag per source for all replicas).
 * Decision, per source row i with actor a = ids[i]:
 *   high, split, the in-place reduced scale, dup, faint, big, wide_old, wide_new: exactly the expressions of emd_refine_decide (same float operations)
 *   oob(p)     = any_c |p_c| > instances_size[a][c] / 2     (NaN compares false, as in torch); active only when do_cull && cull_out_of_bound
 *   original   : kept unless faint | big | wide_old | oob(mean_i)
 *   duplicate  : dup and not (faint | big | wide_new | oob(mean_i))
 *   sample r   : split and not (faint | big | wide_new | oob(p_r)), p_r = R(q^)(exp(scale) * n_r) + mean_i evaluated by the SAME device function the
 *                gather stores positions with, on the same Philox key (seed, source row, replica) or the same caller-supplied normal: the position
 *                that was tested is, bit for bit, the position that is stored.
 *   Caller-supplied normals of this event are `samples` [num_samples, N, 3], indexed by SOURCE ROW (the rank among split sources is not known when
 *   the decision runs): emd_refine_nodes_index writes split_rank[j] = source row on sample rows (0 elsewhere) and the gather is given num_split = N.
 * Sequence:
 *   emd_refine_nodes_decide -> code[N] (bit c = column c) and per-block counts of 4 + num_samples 0/1 columns: 0 original kept, 1 duplicate kept,
 *                              2 source is split, 3 + r sample of replica r kept, 3 + num_samples id outside [0, num_actors)
 *   emd_densify_scan        -> on those columns, at most 8 per call (columns are independent: a caller with more scans them in slices); the totals
 *                              are the event's single host read.  A non-zero bad-id total means: gather nothing.
 *   emd_refine_nodes_index  -> src[M], kind[M] (as emd_refine_index), ids_out[M] = ids[src], split_rank[M], M = keep + sum_r samp_r + dup
 *       group_by_actor = 0: the reference's order: kept originals, kept samples of replica 0, 1, ..., kept duplicates, each in source order;
 *                           segment_start may be NULL and is not written (N == 0 or M == 0: zeroed when given)
 *       group_by_actor = 1: the STABLE sort of that order by actor id (the library's radix sort on the ids, ceil(bits(A - 1) / 9) passes), and
 *                           segment_start[a] = first output row of actor a, segment_start[A] = M.  An actor left with no rows keeps an empty segment.
 *                           Input ids may come in any order.  `workspace`: emd_refine_nodes_index_workspace(M) bytes of scratch.
 *       No atomics on global memory, no host read; every argument is checked before anything is launched (num_actors 1..65536, num_samples 1..13,
 *       the two switches 0 / 1); N == 0 returns EMD_OK with segment_start all zero.
 *   emd_densify_gather      -> as it is, with EMD_DENSIFY_MODE_REFINE. */
typedef struct EmdRefineNodesArgs {
    /* the fields of EmdRefineArgs, same meaning */
    int32_t num_points, do_densify, do_cull, use_split_screen, cull_big, use_cull_screen;
    const float* scaling;
    const float* opacity;
    const float* grad_norm;
    const float* vis_counts;
    const float* max_2Dsize;
    float grad_threshold, size_threshold, split_screen, cull_alpha, cull_size, cull_screen;
    /* the actor part */
    const float* means;            /* [N,3] source positions in the actor's frame */
    const float* rotation;         /* [N,4] source quaternions */
    const int32_t* ids;            /* [N] actor of every row */
    const float* instances_size;   /* [A,3] box extents */
    int32_t num_actors;            /* 1..65536 */
    int32_t num_samples;           /* 1..13 */
    int32_t cull_out_of_bound;     /* 0 / 1 */
    int32_t group_by_actor;        /* 0 / 1 */
    uint64_t seed;                 /* the Philox key the gather will use */
    const float* samples;          /* [num_samples, N, 3] normals by source row to use instead of Philox, or NULL */
} EmdRefineNodesArgs;
int emd_refine_nodes_decide(const EmdRefineNodesArgs* args, int32_t* code /*[N]*/, int32_t* block_counts /*[4 + num_samples, ceil(N / 256)]*/, void* hip_stream);
size_t emd_refine_nodes_index_workspace(int32_t num_out);
int emd_refine_nodes_index(const EmdRefineNodesArgs* args, int32_t num_out, const int32_t* code, const int32_t* block_offsets /*[4 + num_samples, ceil(N / 256)]*/,
                           const int32_t* totals /*[4 + num_samples]*/, int32_t* src, int32_t* kind, int32_t* ids_out, int32_t* segment_start /*[A + 1]*/,
                           int32_t* split_rank /*[M] or NULL*/, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- Adam over all parameter tensors in one launch ---------------------------------------
 * Replaces optimizer.step() of `torch.optim.Adam(l, lr=0.0, eps=1e-15)` (S3Gaussian/scene/gaussian_model.py:188-201,
 * train.py:428; OmniRe builds the same optimiser per class, models/trainers/base.py:213-253): per element
 *   m = m + (1-beta1)(g-m);  v = v beta2 + (1-beta2) g g;  p = p - step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * in torch.optim.Adam's operation order, in place.  The caller supplies the step-dependent scalars (computed in double, as torch
 * does): step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t).  param / grad / exp_avg / exp_avg_sq of one
 * tensor must share one memory layout (they are walked as flat arrays of `numel` floats). */
#define EMD_ADAM_MAX_TENSORS 32
typedef struct EmdAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float step_size, bias_correction2_sqrt, one_minus_beta1, beta2, one_minus_beta2, eps;
    /* ABI 20, optional ("capturable" steps: an optimiser step recorded into a hipGraph must not bake the step count or the learning rate
     * into its launch): with step_dev != NULL the kernel forms step_size = lr_dev[0] / (1 - beta1^t) and bias_correction2_sqrt =
     * sqrt(1 - beta2^t) itself from t = step_dev[0] (the step count AFTER this step's increment, a device float as torch's capturable
     * Adam keeps it) and ignores the two by-value fields; lr_dev must then be non-NULL too. */
    const float* step_dev;
    const float* lr_dev;
} EmdAdamTensor;

typedef struct EmdAdamArgs {
    int32_t num_tensors, reserved;
    EmdAdamTensor tensors[EMD_ADAM_MAX_TENSORS];
} EmdAdamArgs;

int emd_adam_step(const EmdAdamArgs* args, void* hip_stream);

/* ---- ABI 28: exact k nearest neighbours in 3-D, and the embedding regulariser over the neighbour table ---------------------------
 * Replaces `simple_knn._C.distCUDA2` (create_from_pcd's initial scales: mean squared distance to the 3 nearest neighbours,
 * S3Gaussian/scene/gaussian_model.py:152-181) and the `o3d_knn` + `weighted_l2_loss_v2` pair of the fine stage (train.py:326-337).
 *
 * emd_knn: for every point n of pts [N,3] the k nearest OTHER points (1 <= k <= EMD_KNN_MAX_K), rows ascending in d2:
 *   idx [N,k] int32 (may be NULL), d2 [N,k] fp32 (may be NULL), mean_d2 [N] = (d2[n,0] + ... + d2[n,k-1]) / k (may be NULL; k = 3: distCUDA2).
 *   - exact: row n holds the k smallest d2(n,m), m != n.  Self is excluded by index, so coincident points are neighbours at distance 0.
 *   - d2(n,m) = dx*dx + dy*dy + dz*dz in fp32 from the fp32 coordinates (fused multiply-adds).  Which of several equidistant points is
 *     returned is unspecified; the call is deterministic (same input, same output).
 *   - fewer than k other points: the missing slots hold idx = -1, d2 = +inf (and mean_d2 = +inf).
 *   - a point with a NaN or infinite coordinate gets a row of -1 / +inf and is nobody's neighbour.
 * No host synchronisation; `workspace` holds emd_knn_workspace(N, k) bytes (0 is returned for invalid arguments).
 * Method: 30-bit Z-order keys over the finite points' bounding box, the radix sort of the binning stage, leaves of 64 consecutive sorted
 * points and groups of 64 leaves with their min / max corners; a wave owns the 64 queries of one leaf, seeds their candidate lists
 * (registers) from the neighbouring leaves and then visits only the leaves whose box lies nearer than the current k-th distance. */
#define EMD_KNN_MAX_K 32
size_t emd_knn_workspace(int32_t num_points, int32_t k);
int emd_knn(int32_t num_points, int32_t k, const float* pts, int32_t* idx, float* d2, float* mean_d2, void* workspace, size_t workspace_bytes,
            void* hip_stream);
/* The transposed adjacency of idx [N,k] in CSR form: rev_start [N+1], rev_slot [N*k] = the flat positions m*k + j of the entries with
 * idx[m,j] == n, for n = 0 .. N-1 one after the other, ascending inside every n (entries < 0 are left out: rev_start[N] of the N*k slots
 * are written).  Built once per table, so that the regulariser's backward gathers instead of scattering with float atomics. */
size_t emd_knn_reverse_workspace(int32_t num_points, int32_t k);
int emd_knn_reverse(int32_t num_points, int32_t k, const int32_t* idx, int32_t* rev_start, int32_t* rev_slot, void* workspace,
                    size_t workspace_bytes, void* hip_stream);
/* loss[0] = (1 / P) sum over the P pairs with idx[n,j] >= 0 of sqrt(w[n,j] * |e[n] - e[idx[n,j]]|^2 + 1e-20); loss[1] = 1 / P (0 when P = 0).
 * e [N,E] fp32 with E in {4, 8, 16, 32}, 16-byte aligned; w [N,k] or NULL (= 1).  c [N,k] (optional) receives w / sqrt(...) per pair (0 where
 * idx < 0) for the backward.  One launch; the sum is formed in a fixed order through the granule table `scratch`
 * (EMD_EMBED_REG_SCRATCH_WORDS 4-byte words, 8-byte aligned, zero at the first call and left zero by every call, one stream at a time), as
 * emd_l1_loss_ws does: no zero fill, no float atomics. */
#define EMD_EMBED_REG_SCRATCH_WORDS 2048
int emd_embed_reg_forward(int32_t num_points, int32_t k, int32_t embed_dim, const float* e, const int32_t* idx, const float* w, float* c,
                          float* loss /*[2]*/, uint32_t* scratch, void* hip_stream);
/* grad_e[n] (+)= g[0] * inv_pairs[0] * ( sum_j c[n,j] (e[n] - e[idx[n,j]])  +  sum over the slots s = m*k + j of rev(n) of c[s] (e[n] - e[m]) ),
 * both sums gathers in a fixed order: bit-identical from run to run.  g [1] = dL/dloss and inv_pairs [1] = loss[1] of the forward, on the
 * device.  c == NULL: the factors are recomputed from w and e.  accumulate != 0 adds to grad_e, otherwise grad_e is overwritten.
 * No gradient flows to w or to the positions. */
int emd_embed_reg_backward(int32_t num_points, int32_t k, int32_t embed_dim, const float* e, const int32_t* idx, const float* w, const float* c,
                           const int32_t* rev_start, const int32_t* rev_slot, const float* g, const float* inv_pairs, float* grad_e,
                           int32_t accumulate, void* hip_stream);

/* ---- ABI 29: the radix sort of the binning and k-NN stages on its own ------------------------------------------------------------
 * A stable LSD radix sort of (32-bit key, 32-bit value) pairs: `passes` passes of `bits` bits each, from the lowest bit of
 * rel = key - offset (mod 2^32) upwards.  The pairs end ordered by the low passes * bits bits of rel; pairs equal in those bits keep their
 * input order, and the full keys travel with the values.  This is the sort behind the depth sort, the tile sort and the k-NN lists
 * (csrc/radix_sort.h), exported so that it can be tested directly; a caller with pairs to sort may use it as well.
 *   - keys_in == NULL: the pairs start in keys[0] / vals[0].  keys_in != NULL: a COMPACTING sort of keys_in [n]: the value of element i is
 *     i, elements whose key is 0xFFFFFFFF are dropped, and the number kept is written to *count_out (passes >= 1 and count_out required).
 *     A kept element with rel >> range_bits != 0 raises bit 1 (value 2) of *overflow_word (range_bits < 32 requires overflow_word;
 *     the word is only ever OR-ed into, never cleared).
 *   - the element count n is n_cap, or *n_dev when n_dev != NULL (it must not exceed n_cap), read as 0 while *n_dev_overflow != 0
 *     (n_dev_overflow may be NULL).  No host synchronisation.
 *   - keys[0], keys[1], vals[0], vals[1]: n_cap words each, all four distinct; hist: (bits == 9 ? 512 : 256) * ceil(n_cap / 2048) words
 *     of scratch.  Only the first n (compacting: *count_out) positions of a pair are written.
 *   - returns the index (0 or 1) of the pair that holds the result: 0 when passes < 1, else (passes - (keys_in != NULL)) & 1; or a
 *     negative EMD_ERR_*.  Every argument is validated before anything is launched; n_cap == 0 launches nothing.
 *   - 1 <= bits <= 9, passes >= 0, passes * bits <= 32, 0 <= n_cap <= 2^32 - 1 - 2048. */
typedef struct EmdRadixSortArgs {
    const uint32_t* keys_in;
    uint32_t* keys[2];
    uint32_t* vals[2];
    uint32_t* hist;
    int64_t n_cap;
    const uint32_t* n_dev;
    const uint32_t* n_dev_overflow;
    int32_t passes, bits;
    uint32_t offset;
    int32_t range_bits;
    uint32_t* overflow_word;
    uint32_t* count_out;
} EmdRadixSortArgs;
int emd_radix_sort(const EmdRadixSortArgs* args, void* hip_stream);

/* ---- ABI 31 extension (a new entry point and a struct only, so the number stays): the binning stage on its own ------------------------------
 * Everything between the projection kernel and the render kernels (csrc/binning.hip: depth order, duplication, partition by tile, tile ranges,
 * dispatch order) on CALLER-SUPPLIED projection outputs, exported so that the stage can be tested directly, as emd_radix_sort is.  It runs the
 * launcher emd_raster_forward runs, on the same workspaces:
 *   - depth_key [N]: float bits of the view depth of every Gaussian, 0xFFFFFFFF = not visible.
 *   - binrec [N][2]: the projection kernel's record (GeomWs::binrec of csrc/common.h): word 0 = x0 | y0 << 10 | width << 20 | skip-left << 30 |
 *     skip-right << 31 of the tile rectangle, word 1 = height | skip-top << 10 | skip-bottom << 11 (bits from 12 up are not read by the stage).
 *     A visible Gaussian emits width * height (tile, Gaussian) pairs, row-major; width or height 0: visible, no pairs.
 *   - both arrays are copied into geom_ws (device to device, on the stream) and are not written; geom_ws / bin_ws are sized by
 *     emd_raster_workspace_size for (num_gaussians, image_height, image_width, bin_capacity) and need no clearing; `status` is cleared here, as
 *     the projection kernel would, and then holds D, the overflow bits, V (EmdStatus).
 *   - tile_order [T] (T = tiles of the image), or NULL: receives BinWs::tile_order, the dispatch order of the render kernels: a permutation of
 *     0 .. T-1 along which min(list length >> 4, 1023) does not increase; the identity when T > 65 536, num_gaussians == 0 or bin_capacity == 0.
 *   - the sorted list, the ranges and the quadrant masks are then read with emd_raster_export_binning on the same workspaces.
 * Checked on the host before anything is launched (EMD_ERR_INVALID): null args / depth_key / binrec (with num_gaussians > 0) / geom_ws / bin_ws /
 * status, negative num_gaussians or bin_capacity, image sizes below 1, num_gaussians >= 2^28, 1024 or more tiles along an axis, a flag other than
 * EMD_FLAG_WIDE_DEPTH_SORT; a workspace shorter than emd_raster_workspace_size reports is EMD_ERR_WORKSPACE.  No host read-back, no synchronisation.
 * PRECONDITIONS on the device data, which the entry cannot check (the projection kernel guarantees them): every rectangle lies inside the tile
 * grid (x0 + width <= tiles across, y0 + height <= tiles down), and the pairs of all visible Gaussians sum to less than 2^32. */
typedef struct EmdBinningArgs {
    int32_t num_gaussians, image_height, image_width;
    int32_t flags;              /* EMD_FLAG_WIDE_DEPTH_SORT or 0 */
    float   near_plane;         /* the narrow depth sort orders by key - bits(max(near_plane, 0)) */
    int64_t bin_capacity;
    const uint32_t* depth_key;
    const uint32_t* binrec;
    void* geom_ws; size_t geom_bytes;
    void* bin_ws;  size_t bin_bytes;
    EmdStatus* status;          /* device, 16 B */
    uint32_t* tile_order;       /* [T] device out, or NULL */
} EmdBinningArgs;
int emd_raster_binning(const EmdBinningArgs* args, void* hip_stream);

/* ---- ABI 30 extension: segmented row sum with a pinned association (csrc/segsum.h), the deterministic stand-in for per-destination float atomics ----
 * n elements (n = n_cap, or *n_dev <= n_cap when n_dev != NULL) with NON-DECREASING destination ids keys[e] and row indices slots[e].  For every
 * maximal run of equal keys: out[key * out_pitch + f] = sum over the run of rows[slots[e] * row_pitch + f], f < width.  Destinations without a
 * run are not written.  The association depends only on the run's length and an element's position in it: consecutive chunks of
 * EMD_SEG_CHUNK elements, each summed in ascending element order in fp64 from 0.0, the chunk sums added in ascending chunk order in fp64
 * from 0.0, one rounding to fp32.  `partials`: emd_segmented_row_sum_workspace(n_cap, width) bytes of scratch, 8-byte aligned, needs no clearing.
 * 1 <= width <= 32, width <= row_pitch, out_pitch; 0 <= n_cap <= 2^32 - 1 - 2048; no host synchronisation, no atomics. */
#define EMD_SEG_CHUNK 512
typedef struct EmdSegSumArgs {
    const uint32_t* keys;
    const uint32_t* slots;
    const uint32_t* n_dev;
    int64_t n_cap;
    const float* rows;
    int32_t row_pitch, width;
    float* out;
    int32_t out_pitch, reserved;
    double* partials;
    size_t partial_bytes;
} EmdSegSumArgs;
size_t emd_segmented_row_sum_workspace(int64_t n_cap, int32_t width);
int emd_segmented_row_sum(const EmdSegSumArgs* args, void* hip_stream);

/* ---- ABI 30 extension (new entry points and structs only, so the number stays): linear-blend skinning of SMPL pedestrian nodes (csrc/skinning.hip) ----
 * OmniRe's fourth Gaussian class: a pedestrian point moves by a per-point blend of J = 24 joint transforms.  Two launches each way, no atomics:
 * every gradient is a fixed function of the call's inputs (bit-reproducible from run to run, across streams and under hipGraph replay); there is
 * no other mode.  Quaternions are (w, x, y, z); R(q) is the rotation of q / |q|; 3x4 transforms are row-major [r00 r01 r02 t0 | r10 ... | r20 ...].
 *
 * Joint chain (SMPLTemplate.forward, human_body.py:158-181), P instances, `parents` a DEVICE int32[24] with parents[0] = -1, parents[j] < j (an
 * entry outside [-1, j - 1] is held to that range; -1 makes joint j a root):
 *     L_j = [R(theta_j) | joints_j - joints_parent(j)]   (a root: joints_j),   G_root = L_root,   G_j = G_parent(j) L_j,
 *     A_j = [G_j.R | G_j.t - G_j.R joints_j],   and A_j <- A_j o canon_inv_j (affine composition) when canon_inv != NULL.
 * theta [P,24,4] is unnormalised (row 0: the global orientation) and receives the gradient, through the normalisation; joints [P,24,3] and
 * canon_inv [P,24,12] are constants. */
#define EMD_SKIN_JOINTS 24
#define EMD_SKIN_CHUNK 256                 /* most points of a chunk of the point layout */
#define EMD_SKIN_PARTIAL_FLOATS 291        /* one chunk's slab: 24 x 12 sums of dL/dA and 3 of dL/dtrans */
typedef struct EmdJointChainArgs {
    int32_t num_instances, reserved;
    const float* theta;
    const float* joints;
    const int32_t* parents;
    const float* canon_inv;                /* or NULL */
    float* A;                              /* [P,24,12]: written by the forward, not read by the backward */
} EmdJointChainArgs;
int emd_joint_chain_forward(const EmdJointChainArgs* args, void* hip_stream);
/* dL/dA reaches the backward in one of two forms (exactly one is non-NULL): dL_dA [P,24,12] dense, or `partials`, the chunk slabs emd_skin_backward
 * left, with instance_chunk_start int32[P+1] (instance p owns the chunks [start[p], start[p+1]) of the table): the slabs of an instance are added in
 * ASCENDING CHUNK ORDER from 0.0 in fp32, and the sums are also stored to dL_dA_out [P,24,12] / dL_dtrans [P,3] when those are non-NULL.  Then the
 * chain runs in reverse, joint s adding into its parent for s = 23 .. 1 (a parent receives its children in descending joint index), and
 * dL_dtheta [P,24,4] is written in full.  dL_dtheta == NULL: only the sum of the slabs is wanted (theta / joints / parents are not read). */
int emd_joint_chain_backward(const EmdJointChainArgs* args, const float* dL_dA, const float* partials, const int32_t* instance_chunk_start,
                             float* dL_dA_out, float* dL_dtrans, float* dL_dtheta, void* hip_stream);

/* Skinning (transform_means_and_quats, smpl.py:438-532).  For a point with ids[i] = p in [0, P):
 *     T_i = sum_j weights[i,j] A[p,j]                 (fp32, ascending j, from 0.0)
 *     world_mean = T_i.R mean + T_i.t + trans[p]
 *     world_quat = quat_act(quat_mult(m2q(T_i.R), quat_act(quat)))
 *     opacity_out = opacity * valid[p]                (valid: P floats, NULL = all 1)
 * m2q is pytorch3d's matrix_to_quaternion on the blended (not orthogonal) block: q_abs = sqrt(max(0, .)) of 1+m00+m11+m22, 1+m00-m11-m22,
 * 1-m00+m11-m22, 1-m00-m11+m22; the candidate of the largest q_abs (the lowest index on a tie) divided by 2 max(q_abs, 0.1); quat_act is
 * F.normalize (eps 1e-12).  A point with ids[i] < 0 (or >= P) is returned as emd_motion_forward returns a static point: unchanged.
 * The forward walks the points in index order and reads neither `order` nor `chunks`.  The backward is driven by the point layout: `chunks` is a
 * DEVICE int32 [num_chunks, 3] table of (instance or -1, first, count <= EMD_SKIN_CHUNK): chunk c owns the points order[first .. first + count)
 * (order == NULL: the identity), all of that instance; an instance's chunks are consecutive and follow its points in ascending position.  Per-point
 * gradients are stored directly (d_weights only when non-NULL; rows of unbound points get pass-through gradients and zero d_weights); chunk c's
 * sums of weights (x) dL/dT and of dL/dworld_mean, added in ASCENDING POSITION from 0.0 in fp32, are stored to partials[c * 291 ..] (chunks of
 * instance -1 store nothing) for emd_joint_chain_backward.  Every point must lie in exactly one chunk; entries that point outside the call's
 * arrays are skipped, never followed.  Checked on the host: ceil(N / 256) <= num_chunks <= N / 256 + P + 1.  No host synchronisation. */
typedef struct EmdSkinArgs {
    int32_t num_points, num_instances, num_chunks, reserved;
    const float* means;
    const float* quats;
    const float* opacities;
    const int32_t* ids;
    const float* weights;                  /* [N,24] dense, 16-byte aligned */
    const float* A;
    const float* trans;
    const float* valid;                    /* or NULL */
    const int32_t* order;                  /* or NULL */
    const int32_t* chunks;                 /* may be NULL for the forward */
    float* world_means;
    float* world_quats;
    float* opacities_out;
} EmdSkinArgs;
typedef struct EmdSkinGrads {
    const float* g_world_means;
    const float* g_world_quats;
    const float* g_opacities_out;
    float* d_means;
    float* d_quats;
    float* d_opacities;
    float* d_weights;                      /* or NULL */
    float* partials;                       /* [num_chunks, EMD_SKIN_PARTIAL_FLOATS], needs no clearing */
} EmdSkinGrads;
int emd_skin_forward(const EmdSkinArgs* args, void* hip_stream);
int emd_skin_backward(const EmdSkinArgs* args, const EmdSkinGrads* grads, void* hip_stream);

/* ---- ABI 30 extension (new entry points and a struct only, so the number stays): the HexPlane regularisers (csrc/plane_reg.hip) ----
 * compute_regulation of S3Gaussian/scene/gaussian_model.py:745-784 (the K-Planes / 4DGaussians formulation) over all planes of all scales: two
 * launches forward, one backward, no float atomics.  A plane is [1, C, H, W] in channel-last memory, [H][W][C] floats, exactly as EmdHexArgs.planes:
 * planes[s][p] belongs to the pair (a, b) = (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) with W = res[s][a], H = res[s][b]; the spatial planes are p = 0, 1, 3,
 * the time planes p = 2, 4, 5, on which H runs along time.
 *     d1[c,h,w] = x[c,h+1,w] - x[c,h,w]            h in [0, H-2]
 *     d2[c,h,w] = d1[c,h+1,w] - d1[c,h,w]          h in [0, H-3]          (along H only, as the reference)
 *     smooth(P) = sum(d2^2) / (C (H-2) W)          l1(P) = sum(|1 - x|) / (C H W)
 *     tv = sum over scales, p in {0,1,3} of smooth(P)    ts = sum over scales, p in {2,4,5} of smooth(P)    l1 = sum over scales, p in {2,4,5} of l1(P)
 *     loss = plane_tv_weight * tv + time_smoothness_weight * ts + l1_time_planes_weight * l1
 * Forward: out[0..3] = loss, tv, ts, l1 (the terms unweighted).  A lane adds at most EMD_PLANE_REG_SEG squares per accumulator in fp32; from there on
 * every sum is fp64, in a fixed order (lanes in a fixed tree, a plane's workgroups in ascending order, the planes in ascending order), so the four
 * floats are bit-identical from run to run, across streams and under hipGraph replay.  `workspace`: emd_plane_reg_workspace_size(args) bytes,
 * 8-byte aligned, needs no clearing (the size is a function of channels, num_scales and res alone; 0 for arguments the forward would refuse).
 * Backward, with g [1] = dL/dloss on the device and d2 = 0 outside [0, H-3]:
 *     d smooth / d x[c,h,w] = 2 / (C (H-2) W) * ((d2[h] - d2[h-1]) - (d2[h-1] - d2[h-2]))
 *     d l1     / d x[c,h,w] = sign(x - 1) / (C H W),   sign(0) = 0       (time planes start at exactly 1)
 * Both stencils are formed as differences of differences, as written: values that sit within a few percent of 1 subtract exactly.  Every element
 * of every dL_dplanes[s][p] (channel-last like the plane) is WRITTEN exactly once: no zero fill by the caller; spatial planes receive
 * g * plane_tv_weight * d smooth, time planes g * (time_smoothness_weight * d smooth + l1_time_planes_weight * d l1).
 * Neither W * C nor a pointer needs to be a multiple of 16 bytes (4-byte alignment suffices; 16-byte aligned planes with W * C % 4 == 0 take the
 * wide loads).  1 <= channels, res >= 1, H < 3 on any plane (res[s][1], res[s][2] or res[s][3] below 3) is EMD_ERR_INVALID: the reference
 * returns NaN there.  No host synchronisation. */
#define EMD_PLANE_REG_SEG 32               /* rows of H one workgroup owns (it reads 2 more forward, 4 more backward) */
typedef struct EmdPlaneRegArgs {
    int32_t channels, num_scales;
    int32_t res[EMD_HEX_MAX_SCALES][4];          /* per scale: resolution along x, y, z, t */
    const float* planes[EMD_HEX_MAX_SCALES][6];
    float plane_tv_weight, time_smoothness_weight, l1_time_planes_weight, reserved;
    float* out;                                  /* forward: [4] loss, tv, ts, l1 */
    const float* g;                              /* backward: [1] dL/dloss */
    float* dL_dplanes[EMD_HEX_MAX_SCALES][6];    /* backward */
} EmdPlaneRegArgs;
size_t emd_plane_reg_workspace_size(const EmdPlaneRegArgs* args);
int emd_plane_reg_forward(const EmdPlaneRegArgs* args, void* workspace, size_t workspace_bytes, void* hip_stream);
int emd_plane_reg_backward(const EmdPlaneRegArgs* args, void* hip_stream);

/* ---- ABI 30 extension (new entry points and a struct only, so the number stays): the image tail of an OmniRe step (csrc/trainer_loss.hip) ----
 * The per-image affine colour correction (models/trainers/base.py:251-258) and the trainer's image losses (compute_losses, base.py:518-620, with
 * models/losses.py, pytorch_msssim.SSIM(data_range=1, channel=3) and kornia.losses.inverse_depth_smoothness_loss).  Everything is fp32 and
 * channels-last, as the trainer's `outputs`: colour images [H][W][3], scalar images [H][W]; 4-byte alignment suffices (rows of 3 W floats are not
 * 16-byte aligned for odd W).  No float atomics and no second mode: every scalar is a sum of per-workgroup fp64 partials added in a fixed order,
 * every gradient element is WRITTEN exactly once by the pixel that owns it (no zero fill by the caller, nothing scattered), so all outputs are
 * bit-identical from run to run, across streams and under hipGraph replay.  No host synchronisation.
 *
 * Affine colour, one A [3][4] (row-major, on the DEVICE) per image, P = num_pixels:
 *     out[p] = A[:, :3] rgb[p] + A[:, 3]          each row ((a0 r + a1 g) + a2 b) + a3: A = [I | 0] returns rgb bit for bit
 *     dL/drgb[p] = A[:, :3]^T g[p]                dL/dA = sum_p g[p] (x) [rgb[p], 1]     (12 sums: fp64 per chunk of EMD_TRAINER_LOSS_CHUNK pixels,
 *                                                                                         the chunks added in ascending order)
 * emd_affine_backward: dL_drgb or dL_daffine may be NULL (not both); `workspace` (emd_affine_workspace_size(P) bytes, 8-byte aligned, needs no
 * clearing) is read only with dL_daffine. */
size_t emd_affine_workspace_size(int64_t num_pixels);
int emd_affine_forward(int64_t num_pixels, const float* rgb, const float* affine, float* out, void* hip_stream);
int emd_affine_backward(int64_t num_pixels, const float* rgb, const float* affine, const float* dL_dout, float* dL_drgb, float* dL_daffine,
                        void* workspace, size_t workspace_bytes, void* hip_stream);

/* The loss tail.  Write x = rgb, y = gt_rgb, o = opacity, s = sky_mask (0 or 1), t = 1 - s, d = depth, l = lidar_depth, P = H W.  A term is SKIPPED
 * when its weight is 0 or one of its inputs is NULL: its scalar is 0 and it adds nothing to any gradient.  sign(0) = 0 everywhere.
 *   rgb      w_rgb * mean over 3 P of |y - x|                                                      d/dx = sign(x - y) / (3 P)
 *   ssim     w_ssim * (1 - mean over 3 (H-10) (W-10) of map), per channel and per window position (i, j), i < H-10, j < W-10:
 *                filt(u)[i,j] = sum_{a,b < 11} k[a] k[b] u[i+a, j+b],  k[a] = exp(-(a-5)^2 / (2 * 1.5^2)) normalised to sum 1   (no padding)
 *                mu1 = filt(x), mu2 = filt(y), s1 = filt(x^2) - mu1^2, s2 = filt(y^2) - mu2^2, s12 = filt(x y) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2
 *                map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * (2 s12 + C2) / (s1 + s2 + C2)
 *            H < 11 or W < 11 with w_ssim != 0 is EMD_ERR_INVALID.
 *   mask     inputs o, s.  EMD_TL_MASK_BCE: w_mask * mean_P of -[t max(ln o, -100) + (1-t) max(ln(1-o), -100)], d/do = (o - t) / max(o (1-o), 1e-12)
 *            (torch's binary_cross_entropy; o must lie in [0, 1]).  EMD_TL_MASK_SAFE_BCE, with o~ = clip(o, 0, 1) and o^ = clip(o~, safe_limit,
 *            1 - safe_limit): value -max(ln(t ? o~ : 1 - o~), ln safe_limit), d/do = 1 / (1 - o^) where t = 0, -1 / o^ where t = 1: the gradient
 *            survives the clip.  0 < safe_limit < 0.5.
 *   depth    inputs d, l, s.  Over the hit pixels v = (t > 0) and (0.01 < l < upper_bound) and (d > 1e-4): with `normalize` d and l are divided by
 *            upper_bound, then with `inverse` u -> 1 / (u + 1e-5); e = |z| (L1), z^2 (L2) or z^2 / 2 for |z| < 1, else |z| - 1/2 (SMOOTH_L1, beta = 1),
 *            z = d' - l';  value w_depth * sum_v e / max(|v|, 1).  An empty hit set gives 0 and a zero gradient (the reference divides by 0 and
 *            returns NaN).  upper_bound > 0.01.
 *   entropy  input o.  w_entropy * mean_P of -o~ ln o~, o~ = clip(o, 1e-6, 1 - 1e-6); d/do = -(ln o~ + 1) where 1e-6 <= o <= 1 - 1e-6, else 0
 *   smooth   input d.  q = 1 / (d + 1e-5), wx[i,j] = exp(-mean_c |y[i,j,c] - y[i,j+1,c]|), wy likewise down the rows:
 *            w_smooth * [ mean over H (W-1) of |(q[i,j] - q[i,j+1]) wx[i,j]| + mean over (H-1) W of |(q[i,j] - q[i+1,j]) wy[i,j]| ];  no gradient
 *            reaches y.  H < 2 or W < 2 with the term active is EMD_ERR_INVALID.
 * losses [7] = total, rgb, ssim, mask, depth, entropy, smooth (each term weighted; the total is their sum).  dL_drgb [H][W][3], dL_dopacity [H][W]
 * and dL_ddepth [H][W] (each may be NULL) are d total / d input: the sum over the terms that touch the input, zero where none does; dL_dopacity
 * needs opacity, dL_ddepth needs depth.  The caller scales them by its upstream scalar.  `workspace`: emd_trainer_loss_workspace_size(args)
 * bytes (a function of height and width alone; 0 for arguments the call would refuse), 8-byte aligned, needs no clearing.  Every argument is
 * checked before anything is launched; at most five launches (point-wise sums, SSIM forward, the scalars, SSIM backward, dL/ddepth). */
#define EMD_TRAINER_LOSS_CHUNK 1024        /* pixels whose sums one workgroup adds into one fp64 partial per term */
#define EMD_TRAINER_SSIM_TILE 32           /* a workgroup of the SSIM forward owns 32 rows x 32 FLOATS of the [H-10][3 (W-10)] map (channels interleaved) */
#define EMD_TL_MASK_BCE 0
#define EMD_TL_MASK_SAFE_BCE 1
#define EMD_TL_DEPTH_L1 0
#define EMD_TL_DEPTH_L2 1
#define EMD_TL_DEPTH_SMOOTH_L1 2
typedef struct EmdTrainerLossArgs {
    int32_t height, width;
    int32_t mask_type, depth_type;               /* EMD_TL_MASK_*, EMD_TL_DEPTH_* */
    int32_t normalize, inverse;                  /* the depth term's options, 0 or 1 */
    const float* rgb;
    const float* gt_rgb;
    const float* opacity;                        /* or NULL */
    const float* sky_mask;                       /* or NULL */
    const float* depth;                          /* or NULL */
    const float* lidar_depth;                    /* or NULL */
    float w_rgb, w_ssim, w_mask, safe_limit;
    float w_depth, upper_bound, w_entropy, w_smooth;
    float* losses;                               /* [7] */
    float* dL_drgb;                              /* or NULL */
    float* dL_dopacity;                          /* or NULL */
    float* dL_ddepth;                            /* or NULL */
} EmdTrainerLossArgs;
size_t emd_trainer_loss_workspace_size(const EmdTrainerLossArgs* args);
int emd_trainer_loss(const EmdTrainerLossArgs* args, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- ABI 31 extension (new entry points and structs only, so the number stays): VanillaGaussians (csrc/vanilla.hip) ----
 * The per-class dictionary of get_gaussians (OmniRe/models/gaussians/vanilla.py:378-414) in one launch each way.  Everything is fp32, contiguous and
 * 16-byte aligned (camera_center: 4-byte); N = num_points, M = sh_coeffs (1 .. 16), n = degree (0 .. 3, (n + 1)^2 <= M), K = (n + 1)^2.
 *     opacities [N,1] = sigmoid(a)          scales [N,3] = exp(l)          quats_out [N,4] = q / max(|q|, 1e-12)
 *     sh mode (sh_mode = 1, the class's sh_degree > 0):
 *         d = mean - c;  d^ = d / |d|;  pre = sum_{k < K} basis_k(n, d^) coeffs_k,  coeffs = [features_dc, features_rest]
 *         rgbs = clamp(pre + 0.5, 0, 1)        no gradient reaches the means or the camera (the directions are detached)
 *     dc mode (sh_mode = 0, sh_degree == 0):  rgbs = sigmoid(features_dc);  features_rest and camera_center are not read
 * The means themselves are the dictionary's `_means` (no copy).  The arithmetic is that of emd_activations_forward and of emd_sh_forward on
 * dirs = means - camera_center, operation for operation: the outputs carry the same bits.  Of features_rest [N,M-1,3] only the K - 1 rows the
 * degree uses are loaded (none at n = 0; NULL is allowed when M = 1); camera_center [3] is read on the DEVICE.  clamp_mask [N] bytes (or NULL in a
 * forward that no backward follows): bit c set where 0 <= pre_c + 0.5 <= 1, torch's closed-interval rule for the gradient of clamp; the backward
 * reads it instead of evaluating the colour again.
 * Backward, for the upstream g_opacities [N], g_scales [N,3], g_quats [N,4], g_rgbs [N,3], any of which may be NULL and then counts as 0
 * (g_opacities, g_scales and g_rgbs need 4-byte alignment only: autograd hands them over as views at any row offset; g_quats 16-byte):
 *     dL/da = g o (1 - o)        dL/dl_k = g_k s_k        dL/dq = (g - q^ (q^ . g)) / max(|q|, 1e-12)
 *     dL/dcoeffs_k = basis_k g~ for k < K and +0 for K <= k < M, g~ = g_rgbs where the mask bit is set and 0 elsewhere
 *     dc mode: dL/dfeatures_dc = g c (1 - c), dL/dfeatures_rest = +0
 * Row 0 of dL/dcoeffs is dL_dfeatures_dc [N,3], rows 1.. are dL_dfeatures_rest [N,M-1,3]: no concatenated buffer.  Every element of every non-NULL
 * gradient tensor is WRITTEN exactly once (no zero fill by the caller); a NULL gradient tensor is not computed.  No atomics, no second mode, no host
 * synchronisation: all outputs are bit-identical from run to run, across streams and under hipGraph replay.  Every argument is checked before the
 * launch: a NULL required pointer, num_points < 0 or above INT32_MAX - 256 (the kernels index Gaussians as int), a degree outside 0 .. 3,
 * (n + 1)^2 > M, M outside 1 .. 16 or a misaligned tensor is EMD_ERR_INVALID.  num_points == 0 launches nothing. */
typedef struct EmdVanillaArgs {
    int32_t num_points, sh_coeffs;               /* N, M */
    int32_t degree, sh_mode;                     /* n; 1 = sh mode, 0 = dc mode */
    const float* means;                          /* [N,3] */
    const float* log_scales;                     /* [N,3] */
    const float* quats;                          /* [N,4] */
    const float* opacity_logits;                 /* [N] */
    const float* features_dc;                    /* [N,3] */
    const float* features_rest;                  /* [N,M-1,3], or NULL when M = 1 */
    const float* camera_center;                  /* [3], device */
    float* opacities;                            /* forward: [N] */
    float* scales;                               /* forward: [N,3] */
    float* quats_out;                            /* forward: [N,4] */
    float* rgbs;                                 /* forward: [N,3] */
    uint8_t* clamp_mask;                         /* [N]: written by the forward, read by the backward (sh mode) */
    const float* g_opacities;                    /* backward: upstream gradients, each or NULL */
    const float* g_scales;
    const float* g_quats;
    const float* g_rgbs;
    float* dL_dopacity_logits;                   /* backward: [N], each or NULL */
    float* dL_dlog_scales;                       /* [N,3] */
    float* dL_dquats;                            /* [N,4] */
    float* dL_dfeatures_dc;                      /* [N,3] */
    float* dL_dfeatures_rest;                    /* [N,M-1,3] */
} EmdVanillaArgs;
int emd_vanilla_forward(const EmdVanillaArgs* args, void* hip_stream);
int emd_vanilla_backward(const EmdVanillaArgs* args, void* hip_stream);

/* The regularisers of compute_reg_loss (the same file).  With s = exp(l), smax / smin over the three columns, V = {i : radii[i] > 0} and
 * R = max_gauss_ratio, terms [4] = sharp_shape, flatten, sparse, max_s_square (each weighted):
 *     sharp_shape   w_sharp * mean_N (max(smax / smin, R) - R)
 *                   gradient only where smax / smin > R: +ratio / N to l of the largest column, -ratio / N to the smallest; equal largest
 *                   (smallest) columns share it evenly (torch.amax / amin)
 *     flatten       w_flatten * mean_N |clamp(smin, 0, 30)|
 *                   smin / N to l of the smallest column where smin < 30; among equal columns the LOWEST index takes all (torch.min with indices)
 *     max_s_square  w_max_s_square * mean_N smax^2
 *                   2 smax^2 / N to l of the largest column; among equal columns the lowest index takes all
 *     sparse        w_sparse * mean_V -(o~ ln o~ + (1 - o~) ln(1 - o~)),  o~ = clamp(sigmoid(a), 1e-6, 1 - 1e-6)
 *                   d/da = -a o (1 - o) / |V| inside the clip (ln((1 - o~) / o~) = -a there), 0 outside, 0 off V; |V| = 0: the term is 0 with a
 *                   zero gradient (the reference drops its key after a host read of |V|).  1 - o is formed as sigmoid(-a), without cancellation.
 * A term whose weight is 0 is SKIPPED: its value is 0 and it adds nothing to a gradient; so is the sparse term when opacity_logits or radii is NULL.
 * Forward: one workgroup per EMD_VANILLA_REG_CHUNK Gaussians writes four fp64 sums and the chunk's visible count; one workgroup then adds the chunks
 * in a fixed order, writes terms and keeps 1 / N and 1 / max(|V|, 1) at the head of the workspace.  Backward (one launch, the forward's workspace,
 * g [4] = the upstream scalar of each term on the device): every element of dL_dlog_scales [N,3] and, when not NULL, of dL_dopacity_logits [N] is
 * WRITTEN exactly once.  `workspace`: emd_vanilla_reg_workspace_size(N) bytes (a function of N alone; 0 for N < 1 or above INT32_MAX - 256), 8-byte aligned, never cleared.
 * 4-byte alignment suffices for the tensors.  No float atomics, no host synchronisation: values and gradients are fixed functions of the inputs.
 * num_points < 1 (a mean over nothing) or above INT32_MAX - 256, a NULL log_scales / terms / g / dL_dlog_scales or max_gauss_ratio <= 0 is EMD_ERR_INVALID. */
#define EMD_VANILLA_REG_CHUNK 1024         /* Gaussians whose sums one workgroup adds into one fp64 partial per term */
typedef struct EmdVanillaRegArgs {
    int32_t num_points, reserved;
    const float* log_scales;                     /* [N,3] */
    const float* opacity_logits;                 /* [N] or NULL */
    const int32_t* radii;                        /* [N] or NULL */
    float w_sharp, max_gauss_ratio, w_flatten, w_sparse;
    float w_max_s_square, reserved1;
    float* terms;                                /* forward: [4] */
    const float* g;                              /* backward: [4] */
    float* dL_dlog_scales;                       /* backward: [N,3] */
    float* dL_dopacity_logits;                   /* backward: [N] or NULL */
} EmdVanillaRegArgs;
size_t emd_vanilla_reg_workspace_size(int32_t num_points);
int emd_vanilla_reg_forward(const EmdVanillaRegArgs* args, void* workspace, size_t workspace_bytes, void* hip_stream);
int emd_vanilla_reg_backward(const EmdVanillaRegArgs* args, const void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- (ABI 31, compatible extension) SMPLNodes: k-NN inside segments and the neighbour-std regulariser ----------------------------------------
 * The reference's smpl.py is not at hand; what follows is the maintainers' reading of its k-NN regulariser (reg.knn_reg, after GART), stated as
 * formulas and pinned by tests/neighbour_std_ref.py (DESIGN.md section 8.19 names the points where the reading could be wrong).
 *
 * emd_knn_segments: emd_knn restricted to segments.  Segment s owns the rows [segment_start[s], segment_start[s+1]) of pts [N,3]; the table
 * [S+1] ascends, lives on the device and is read there (no host read); its entries are clamped to [0, N].
 *   - row n holds the k smallest d2(n,m) over the OTHER rows m of n's own segment, ascending, as GLOBAL row numbers; d2 is emd_knn's fp32
 *     expression; self is excluded by index.
 *   - among equidistant candidates the LOWER row number comes first (stricter than emd_knn).
 *   - missing slots hold idx = -1, d2 = +inf: a segment of fewer than k + 1 rows (sizes 1 and 2 included), a row outside every segment, and a
 *     row with a non-finite coordinate, which is also nobody's neighbour.
 *   - deterministic; idx or d2 may be NULL (not both); 1 <= k <= EMD_KNN_MAX_K; every argument is validated before anything is launched and
 *     N == 0 launches nothing.  No workspace, no sort, no atomics: brute force per segment, one wave per 64 consecutive rows. */
int emd_knn_segments(int32_t num_points, int32_t num_segments, int32_t k, const float* pts, const int32_t* segment_start, int32_t* idx, float* d2,
                     void* hip_stream);

/* emd_neighbour_std_forward / _backward.  idx [N,k] holds the k = K - 1 OTHERS of every point's group (the point itself is implicit:
 * knn_points(x, x, K) returns it first); entries outside [0, N) are empty slots.  Up to EMD_NSTD_MAX_BLOCKS blocks x_b [N,C_b] fp32 contiguous,
 * 1 <= C_b <= EMD_NSTD_MAX_COLS, each with an activation a_b and a weight w_b.
 * Forward.  G(n) = {n} u {idx[n,j] valid}, g = |G(n)|.  Per column c of block b, in fp32 and in this order:
 *     v_m = a_b(x_b[m,c]);  d_m = v_m - v_n for m in the order n (d = 0), then ascending j;  mu = (sum d_m) / g;
 *     sigma = sqrt(sum (d_m - mu)^2 / (g - 1)), the sum starting with the point's own term;  sigma = 0 when g < 2
 *     terms[b] = w_b / (N C_b) * sum_n sum_c sigma        (= (a_b(x_b)[cat(self, idx)].std(dim=1).mean() * w_b)
 * The shift by the group's first member is part of the contract: a group whose members are bit-identical in a column gives sigma == 0 exactly and
 * a gradient of exactly 0 (a mean-first form would not: (x + x + x) / 3 != x in fp32).  exp is expf, sigmoid is 1 / (1 + expf(-x)); no fused
 * multiply-adds.  The sigmas are added in fp64: per workgroup one partial per block, the partials in workgroup order by the last workgroup to
 * arrive (an integer ticket; nobody waits).  One launch, no float atomics, no zero fill.  A block with w_b == 0 is SKIPPED: terms[b] = 0, its
 * x / dx are not touched.  The forward leaves (mu, 1 / ((g - 1) sigma)) -- 0 where sigma is 0 -- per point and active column in `stash`
 * ([N][T][2] floats, T = the columns of the blocks with w_b != 0, 8-byte aligned).
 * Backward (a gather, one launch; every element of the active blocks' dx written exactly once):
 *     dx_b[j,c] = a_b'(x_b[j,c]) * (g_terms[b] w_b / (N C_b)) * sum over the groups n containing j of (d^n_j - mu_n) / ((g_n - 1) sigma_n)
 * with terms of sigma_n == 0 equal to 0 and the groups in the order n = j, then the owners of rev(j)'s slots (emd_knn_reverse) ascending.
 * Values and gradients are fixed functions of the inputs: bit-identical from run to run, across streams and under graph replay.
 * `workspace`: emd_neighbour_std_workspace_size() bytes, 8-byte aligned, its first 16 bytes zero at the first call and left zero by every call
 * (one stream at a time).  N == 0 or no active block: terms are zeroed, nothing else is launched. */
#define EMD_NSTD_MAX_BLOCKS 8
#define EMD_NSTD_MAX_COLS 64
#define EMD_NSTD_ACT_IDENTITY 0
#define EMD_NSTD_ACT_EXP 1
#define EMD_NSTD_ACT_SIGMOID 2
typedef struct EmdNeighbourStdArgs {
    int32_t num_points, k, num_blocks, reserved;
    const int32_t* idx;                          /* [N,k] */
    const int32_t* rev_start;                    /* backward: [N+1] */
    const int32_t* rev_slot;                     /* backward: [N*k] */
    const float* x[EMD_NSTD_MAX_BLOCKS];         /* [N,C_b] */
    int32_t cols[EMD_NSTD_MAX_BLOCKS], act[EMD_NSTD_MAX_BLOCKS];
    float weight[EMD_NSTD_MAX_BLOCKS];
    float* stash;                                /* forward: written; backward: read */
    float* terms;                                /* forward: [num_blocks] */
    const float* g_terms;                        /* backward: [num_blocks], the upstream scalar of each term, on the device */
    float* dx[EMD_NSTD_MAX_BLOCKS];              /* backward: [N,C_b] */
} EmdNeighbourStdArgs;
size_t emd_neighbour_std_workspace_size(void);
int emd_neighbour_std_forward(const EmdNeighbourStdArgs* args, void* workspace, size_t workspace_bytes, void* hip_stream);
int emd_neighbour_std_backward(const EmdNeighbourStdArgs* args, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* EMD_RASTER_H */
