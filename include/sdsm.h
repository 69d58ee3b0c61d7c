/*
 * sdsm.h -- C ABI of the MI355X-native SuperDSM hot path (libsdsm_hip.so).
 *
 * The reference (BMCV/SuperDSM @ 2024_08_07) has no FFI for this path: its only native boundary is MKL via
 * ctypes (superdsm/_mkl.py:1-8, superdsm/_libs/sparse_dot_mkl/_mkl_interface.py:6-135) and cvxopt's C
 * extension behind `cvxopt.solvers.cp` (superdsm/dsm.py:488).  This header is the boundary a maintainer
 * would bind instead (see INTEGRATION.md for the ctypes stub): it replaces, per entry point,
 *
 *   sdsm_preprocess            Preprocessing.process                superdsm/preprocess.py:39-68
 *   sdsm_image_prepare         the candidate-independent half of    superdsm/objects.py:95-128
 *                              Object.get_cvxprog_region (EDT(y<=0) <= margin, per-atom extents)
 *   sdsm_plan_* / sdsm_batch_* compute_objects / _compute_object    superdsm/objects.py:177-284
 *                              cvxprog + Energy + CP.solve          superdsm/objects.py:361-412, dsm.py:253-490
 *                              SmoothMatrixFactory.get              superdsm/dsm.py:137-237
 *   sdsm_dsm_config            DSM_CONFIG_DEFAULTS                  superdsm/dsmcfg.py:6-21
 *
 * Conventions: extern "C", plain pointers and sizes, no C++ / torch types.  Every function returns 0 on
 * success and a negative sdsm_status on failure; sdsm_last_error() returns a thread-local message.
 * All device buffers are allocated and freed by the caller (PyTorch-ROCm tensors on the Python side) and
 * passed as raw device pointers; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Calls on one stream are ordered; nothing here synchronises the device except where stated.
 * There is no CPU backend: without a HIP device every compute entry point fails with SDSM_ERR_DEVICE.
 */
#ifndef SDSM_H
#define SDSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDSM_VERSION 200

typedef enum {
    SDSM_OK = 0,
    SDSM_ERR_ARGUMENT = -1,
    SDSM_ERR_DEVICE = -2,      /* HIP runtime error / no device */
    SDSM_ERR_WORKSPACE = -3,   /* caller-provided buffer too small */
    SDSM_ERR_UNSUPPORTED = -4
} sdsm_status;

/* Hyper-parameters of the operator: DSM_CONFIG_DEFAULTS (dsmcfg.py:6-21) minus the keys that are
 * meaningless on the GPU (cachesize, cachetest, smooth_mat_max_allocations, smooth_mat_dtype = float32
 * construction is always used, cp_timeout is replaced by the iteration cap). */
typedef struct {
    double scale;                      /* dsm/scale (1000) */
    double epsilon;                    /* dsm/epsilon (1.0) */
    double alpha;                      /* dsm/alpha */
    double smooth_amount;              /* dsm/smooth_amount, sigma_G; +inf = elliptical models only (c2freganal.py:126) */
    double gaussian_shape_multiplier;  /* dsm/gaussian_shape_multiplier (2) */
    double background_margin;          /* dsm/background_margin */
    int32_t smooth_subsample;          /* dsm/smooth_subsample */
    int32_t init_elliptical;           /* dsm/init == 'elliptical' */
    int32_t max_iters;                 /* Newton iteration cap per solve (100 = cvxopt's maxiters) */
    int32_t flags;                     /* bit 0: no "single positive pixel" shortcut (objects.py:184-191) -- for callers that mirror a direct
                                          cvxprog call, e.g. the normalised energies of c2freganal.py:58-79 */
} sdsm_dsm_config;

/* One candidate's result (objects.py:198-211).  128 bytes, written by the device. */
typedef struct {
    double energy;          /* psi(result), unscaled (objects.py:208) */
    double theta[6];        /* a1,a2,a3,b1,b2,c in full-image-normalised coordinates (dsm.py:49-54) */
    double energy_ell;      /* psi of the elliptical solution the DSM solve started from */
    int32_t status;         /* sdsm_cand_status */
    int32_t flags;          /* bit0: elliptical retry from the moment initialisation (objects.py:337-355) */
    int32_t n_pixels;       /* N = region pixels */
    int32_t n_deform;       /* M = deformation parameters (grid points) */
    int32_t iters_ell, iters_dsm;   /* Newton iterations */
    int32_t evals_value;    /* pixel passes that computed psi only */
    int32_t evals_full;     /* pixel passes that computed psi, gradient and Hessian */
    int32_t on_boundary;    /* S > 0 anywhere on the 1-px pad ring (objects.py:209) */
    int32_t fg_r0, fg_c0, fg_h, fg_w;   /* bounding box of the foreground fragment; fg_h == 0: empty */
    int32_t n_positive;     /* region pixels with y > 0 */
    int32_t n_negative;     /* region pixels with y < 0 (C2F: a region whose pixels are all positive or all negative has no energy, c2freganal.py:67-68) */
    int32_t reserved;
} sdsm_record;

typedef enum {
    SDSM_CAND_OPTIMAL = 0,      /* is_optimal = True */
    SDSM_CAND_FALLBACK = 1,     /* DSM solve failed, elliptical result returned (objects.py:406-410) */
    SDSM_CAND_TRIVIAL = 2,      /* single positive pixel (objects.py:184-191): energy 0, is_optimal False */
    SDSM_CAND_ERROR = 3,        /* CvxprogError (objects.py:351-353) or malformed G~ (dsm.py:194) */
    SDSM_CAND_UNSUPPORTED = 4,  /* exceeds an implementation limit; elliptical result returned */
    SDSM_CAND_GIVEN_UP = 5      /* scheduling, not arithmetic: the workgroup group of a very large region waited too long for a member (GPU
                                   oversubscribed by other work) and gave the candidate up; no result.  Solve it again with groups
                                   disabled (sdsm_plan_set_latency_mode(plan, 2)); superdsm_amd.objects.compute_objects does. */
} sdsm_cand_status;

/* Per-atom statistics written by sdsm_image_prepare: for label l (1..n_atoms) six int32 at [6*l]:
 * area (pixels with atoms == l, y_mask and EDT(y<=0) <= margin), rmin, rmax, cmin, cmax, reserved. */
#define SDSM_ATOM_STATS_STRIDE 6

/* ---- library --------------------------------------------------------------------------------- */
int sdsm_version(void);
const char *sdsm_last_error(void);
int sdsm_device_count(void);
int sdsm_set_device(int device);
/* Blocks until all work queued on `stream` has finished. */
int sdsm_stream_synchronize(void *stream);

/* Gaussian PSF of G~ (dsm.py:137-142, float32 cast dsm.py:226).  Host function.  Returns k (the PSF is
 * k x k); writes k*k floats if `out` != NULL. */
int sdsm_psf(double sigma, double multiplier, float *out);

/* ---- preprocessing (preprocess.py:39-68) ------------------------------------------------------- */
size_t sdsm_preprocess_workspace_bytes(int H, int W, double sigma1, double sigma2);
/* d_g: H*W float64 in [0,1] (pipeline.py:192), d_y: H*W float64 out.  Device pointers. */
int sdsm_preprocess(const double *d_g, int H, int W, double sigma1, double sigma2, double offset_clip,
                    int lower_clip_mean, double *d_y, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- per-image preparation --------------------------------------------------------------------- */
size_t sdsm_image_workspace_bytes(int H, int W);
/* d_y float64 H*W, d_y_mask uint8 H*W (NULL = all True), d_atoms int32 H*W (labels 1..n_atoms, 0 = none).
 * Outputs: d_valid uint8 H*W = y_mask & (EDT(y <= 0) <= margin)   (objects.py:126-127; image.py:82)
 *          d_atom_stats int32 (n_atoms+1)*SDSM_ATOM_STATS_STRIDE. */
int sdsm_image_prepare(const double *d_y, const uint8_t *d_y_mask, const int32_t *d_atoms, int H, int W,
                       double background_margin, int n_atoms, uint8_t *d_valid, int32_t *d_atom_stats,
                       void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- batch of candidates (one compute_objects call) ------------------------------------------- */
typedef struct sdsm_plan sdsm_plan;   /* host-side plan: offsets into the workspace, launch order */

/* atom_stats: HOST copy of d_atom_stats.  offsets[n+1]/labels[]: footprints in CSR form (objects.py:53). */
sdsm_plan *sdsm_plan_create(int H, int W, int n_atoms, const int32_t *atom_stats, const sdsm_dsm_config *cfg,
                            int n, const int32_t *offsets, const int32_t *labels);
/* The same for candidates of SEVERAL images in one plan (1 <= n_images <= 16): one launch then fills the GPU even when the batches
 * of the single images are small (the generations of globalenergymin.py:228-263 are tens of candidates; an image set as in
 * examples/NIH3T3).  H / W / n_atoms / atom_stats: one entry per image; image_of[i]: the image of candidate i (NULL: all 0); the
 * labels of a footprint refer to that image's atoms.  All images share the hyper-parameters. */
sdsm_plan *sdsm_plan_create_multi(int n_images, const int32_t *H, const int32_t *W, const int32_t *n_atoms, const int32_t *const *atom_stats,
                                  const sdsm_dsm_config *cfg, int n, const int32_t *offsets, const int32_t *labels, const int32_t *image_of);
void sdsm_plan_destroy(sdsm_plan *plan);
size_t sdsm_plan_workspace_bytes(const sdsm_plan *plan);
size_t sdsm_plan_mask_bytes(const sdsm_plan *plan);       /* total size of the bit-packed region-bbox masks */
/* Per candidate i: mask_info[4*i..] = r0, c0, h, w of the region bounding box its mask bits cover (row-major,
 * LSB-first within uint32 words), mask_offset[i] = byte offset into the mask buffer; n_pixels[i] = N. */
int sdsm_plan_describe(const sdsm_plan *plan, int32_t *mask_info, int64_t *mask_offset, int32_t *n_pixels);
/* Algorithmic bytes of the setup phase (crop reads + writes), for the roofline bookkeeping. */
int64_t sdsm_plan_total_pixels(const sdsm_plan *plan);

/* Copies the plan tables into the workspace (H2D, asynchronous on `stream`). */
int sdsm_batch_upload(const sdsm_plan *plan, void *d_workspace, size_t workspace_bytes, void *stream);
/* Region crops, G~ rows, elliptical + DSM solves, masks, records.  Everything stays on the device:
 * d_records: n * sizeof(sdsm_record); d_masks: sdsm_plan_mask_bytes(); d_xi (optional, may be NULL):
 * float64, sdsm_plan_xi_count() entries, candidate i's xi at xi_offset[i] (debug / tests). */
int sdsm_batch_launch(const sdsm_plan *plan, const double *d_y, const int32_t *d_atoms, const uint8_t *d_valid,
                      void *d_workspace, size_t workspace_bytes, sdsm_record *d_records, uint32_t *d_masks,
                      double *d_xi, void *stream);
/* d_y / d_atoms / d_valid: HOST arrays of n_images device pointers (plans of sdsm_plan_create_multi). */
int sdsm_batch_launch_multi(const sdsm_plan *plan, const double *const *d_y, const int32_t *const *d_atoms, const uint8_t *const *d_valid,
                            void *d_workspace, size_t workspace_bytes, sdsm_record *d_records, uint32_t *d_masks, double *d_xi, void *stream);
int64_t sdsm_plan_xi_count(const sdsm_plan *plan);
/* Workspace layout for inspection (parity tests of the crops / grid / G~ rows).  out[16], byte offsets into the
 * workspace: 0 cand table, 1 cand state (M, status, ...), 2 crop_y f64, 3 crop_rc u32, 4 crop_cc u32 (setup only: raster order; unused for regions whose setup state is held in LDS),
 * 5 ell_meta u32 (row entries | Hessian entries << 16), 6 grid u32, 7 ell_idx u16, 8 ell_w f32; then 9 zcap (entries
 * per row, a multiple of 4), 10 k, 11 sizeof(cand entry), 12 total_pixels, 13 total_ell entries, 14 sizeof(cand state);
 * 15 reserved.  Candidate i's blocks start at crop offset sum(n_pixels[:i]), G~ offset that * zcap -- entry s of crop
 * position p at element ((s / 4) * N + p) * 4 + s % 4 of the candidate's block -- and grid offset xi_offset[i]. */
int sdsm_plan_layout(const sdsm_plan *plan, int64_t *out);
/* Scheduling of one batch, mode =
 *   0  throughput (default): every candidate whose system fits is solved by a 192- or 256-thread workgroup, two to four per compute
 *      unit -- most candidate solves per second when the GPU is full (plans over several images, several batches in flight); only
 *      regions of more than max(8192, pixels of all candidates of the plan / 1024) pixels are solved by a GROUP of cooperating
 *      512-thread workgroups (the largest first, until the members add up to 256);
 *   1  latency: regions of more than 3072 pixels are solved by groups of 2-4 workgroups too (same member budget), which shortens
 *      the slowest candidates and with them the wall clock of a single batch (the reference waits for all candidates of an image
 *      before the set-cover step, globalenergymin.py:131-137);
 *   2  no groups: every candidate by a single workgroup (slow for very large regions; the way to solve candidates again whose
 *      group was given up, SDSM_CAND_GIVEN_UP).
 * Results do not depend on the mode.  It changes the launch lists and the workspace size: call it before
 * sdsm_plan_workspace_bytes / sdsm_batch_upload; a launch on a workspace uploaded before the change fails with SDSM_ERR_ARGUMENT. */
int sdsm_plan_set_latency_mode(sdsm_plan *plan, int mode);
/* What the current mode schedules per candidate (host only, diagnostics and tests): group_members[i] = workgroups of the group that
 * solves candidate i (0: a single workgroup), rows_workgroups[i] = workgroups that build its rows of G~ (0: the setup workgroup itself).
 * Either pointer may be NULL. */
int sdsm_plan_schedule(const sdsm_plan *plan, int32_t *group_members, int32_t *rows_workgroups);
/* The launch lists of the plan in its current mode (host only, diagnostics and tests): spans = (first, count) of the seven lists
 * [all candidates, largest first | those whose bound on M admits more than class 1 | more than class 2 | members of the workgroup groups |
 * workgroups that build rows of G~ | setup by the small class | setup by the large class] in one array of entries; order, if not NULL,
 * receives that array (as many int32 as the counts add up to; member lists hold candidate | member << 24). */
int sdsm_plan_lists(const sdsm_plan *plan, int32_t spans[14], int32_t *order);
/* What the plan's kernels are given in its current mode, as raw bytes (host only, diagnostics and tests; read-only).  params receives the
 * kernel arguments laid over a NULL workspace (params_bytes must be 856, the size of the argument struct): every pointer into the workspace
 * then holds its block's byte offset, the image pointers are NULL, so the one blob carries all offsets and all scalars.  cand receives the
 * candidate descriptors (cand_bytes must be 112 times the plan's candidates).  A size that differs is SDSM_ERR_ARGUMENT. */
int sdsm_plan_image(const sdsm_plan *plan, void *params, size_t params_bytes, void *cand, size_t cand_bytes);
/* The solve class of every candidate in the plan's current mode (host only, diagnostics and tests), given what the setup kernel found for it
 * (status, M and env_size of its state): 0 class 1, 1 class 1b, 2 class 2, 3 class 2b, 4 the global-memory class, 5 / 6 / 7 a workgroup
 * group with the LDS layout of class 2 / of class 2b / the light layout (at most 288 unknowns and 12 400 envelope doubles: its members
 * share their compute units with class 1), -1 none (status != 0).  Results do not depend on the class. */
int sdsm_plan_solve_classes(const sdsm_plan *plan, const int32_t *status, const int32_t *M, const int32_t *env_size, int32_t *cls);
/* Diagnostic, process-wide, taken by every following launch and by sdsm_plan_solve_classes: the envelope limit (doubles) of the light
 * group class, in every plan with groups; 0 = no light groups, negative = the default (12 400 in plans of more than 1024 candidates -- a class-1 slot beside a member
 * helps only where class-1 candidates outnumber the chip's class-1 slots --, none in smaller plans), more than 12 400: SDSM_ERR_ARGUMENT. */
int sdsm_set_light_envelope_limit(int doubles);
int sdsm_plan_xi_offsets(const sdsm_plan *plan, int64_t *xi_offset);

/* ---- post-processing, per-object work (superdsm/postprocess.py:254-337) ------------------------------------- */
/* One object's results.  64 bytes, written by the device. */
typedef struct {
    double contrast;        /* (interior_mean + eps) / (exterior_mean + eps)                     postprocess.py:254-266 */
    double interior_mean;   /* mean of g / g.std() over the object's mask */
    double exterior_mean;   /* weighted mean over the exterior neighbourhood */
    double fg_mean, fg_std; /* mean / population std of the smoothed intensities over the mask   postprocess.py:323-325 */
    int32_t area;           /* mask pixels */
    int32_t status;         /* 0 ok, 1 boundary list too long and no pool slot, 2 empty mask, 3 ok, no refinement requested */
    int32_t r0, c0, h, w;   /* bounding box of the refined mask (h == 0: empty) */
} sdsm_post_record;
/* d_g: raw intensities (H*W float64); d_gs: Gaussian-smoothed intensities used by the mask refinement (postprocess.py:165);
 * d_bg: background_mask uint8 (postprocess.py:152-155).  Objects: d_boxes n*4 int32 (r0, c0, h, w of each fragment), fragments
 * bit-packed (row-major, LSB first in uint32 words) at d_bits + d_bits_off[i] (in words).  Outputs: d_out n records; the refined
 * masks over the windows box +- max_distance (clamped to the image), bit-packed at d_new_bits + d_new_off[i] (only written when
 * max_distance > 0 and stdamp > 0; holes are filled by sdsm_post_fill_holes, over these windows).  d_boundary_pool / d_bpool_off (may be NULL): global
 * boundary lists for objects whose mask boundary exceeds 12288 pixels (d_bpool_off[i] < 0: none).  inv_gstd = 1 / g.std(). */
int sdsm_post_objects(const double *d_g, const double *d_gs, const uint8_t *d_bg, int H, int W, int n, const int32_t *d_boxes,
                      const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_new_off, uint32_t *d_new_bits,
                      uint32_t *d_boundary_pool, const int64_t *d_bpool_off, double exterior_scale, double exterior_offset,
                      double contrast_epsilon, double inv_gstd, int max_distance, double stdamp, sdsm_post_record *d_out, void *stream);
/* sdsm_post_objects for the objects of up to SDSM_MAX_SET_IMAGES images in ONE launch (one workgroup per object).  The per-image inputs
 * move into a HOST table of sdsm_post_image; the objects of image 0 come first (n_objects of them), then those of image 1, and so on.
 * Every per-object array (d_boxes, d_bits_off, d_bits, d_new_off, d_new_bits, d_boundary_pool, d_bpool_off, d_out) runs over the
 * objects of the whole set with the meaning and formats of sdsm_post_objects; a box is in its own image's coordinates.  The shared
 * parameters hold for every image.  Per object, byte-equal to sdsm_post_objects on its image alone. */
typedef struct {
    const double *d_g;      /* raw intensities, H*W float64 */
    const double *d_gs;     /* smoothed intensities of the mask refinement */
    const uint8_t *d_bg;    /* background_mask */
    int32_t H, W;           /* 1 .. 65535 */
    double inv_gstd;        /* 1 / g.std() */
    int32_t n_objects;      /* >= 0 */
    int32_t reserved;
} sdsm_post_image;
int sdsm_post_objects_multi(const sdsm_post_image *images, int n_images, const int32_t *d_boxes, const int64_t *d_bits_off,
                            const uint32_t *d_bits, const int64_t *d_new_off, uint32_t *d_new_bits, uint32_t *d_boundary_pool,
                            const int64_t *d_bpool_off, double exterior_scale, double exterior_offset, double contrast_epsilon,
                            int max_distance, double stdamp, sdsm_post_record *d_out, void *stream);
/* ---- post-processing, the exact bit problems: background mask, hole filling, glare test ------------------------------------------
 * All three compute what SciPy computes on the host, bit for bit (superdsm/postprocess.py:152-155, :269-286, :336).  Objects and
 * windows are bit-packed as sdsm_post_objects takes them (row-major, LSB first, whole uint32 words per object). */
#define SDSM_POST_MAX_BG_RADIUS 32
#define SDSM_POST_MAX_GLARE_LAYERS 32
/* One image of sdsm_post_background_multi.  d_work: 5*H*W bytes of scratch, int32-aligned: H*W int32 of paint, then H*W uint8 of row
   distances (contents ignored and destroyed). */
typedef struct {
    uint8_t *d_bg;          /* out: background_mask, H*W uint8 (0 / 1) */
    int32_t *d_work;
    int32_t H, W;           /* 1 .. 65535, H * W < 2^31 */
    int32_t n_objects;      /* >= 0 */
    int32_t reserved;
} sdsm_post_bg_image;
/* background_mask of every image of a set: the complement of the objects' boxes painted in their order (an object assigns its whole
 * box, so the last one decides where boxes overlap), eroded by disk(radius) with the outside of the image as background.  The objects
 * of image 0 come first in d_boxes / d_bits_off (n_objects of them), then those of image 1, and so on; parts of a box outside its
 * image are ignored.  0 <= radius <= SDSM_POST_MAX_BG_RADIUS; radius 0 gives the plain complement. */
int sdsm_post_background_multi(const sdsm_post_bg_image *images, int n_images, const int32_t *d_boxes, const int64_t *d_bits_off,
                               const uint32_t *d_bits, int radius, void *stream);
/* scipy.ndimage.binary_fill_holes (default structure: 4-connected background) of n bit-packed windows, one workgroup each: window i
 * has d_dims[2i] x d_dims[2i+1] pixels at word d_off[i] of d_in and of d_out (d_out may be d_in).  A window of more than 4096 words
 * of whole-word rows (h * ceil(w / 32)) is flooded in global memory and needs 2 * h * ceil(w / 32) words at d_ws + d_ws_off[i]
 * (d_ws_off[i] < 0, or d_ws NULL: none); d_status[i] = 0 filled, 1 workspace missing (the window is not written). */
int sdsm_post_fill_holes(int n, const int32_t *d_dims, const int64_t *d_off, const uint32_t *d_in, uint32_t *d_out, uint32_t *d_ws,
                         const int64_t *d_ws_off, int32_t *d_status, void *stream);
/* The glare test of the objects of a set (one workgroup per object; table and object order as for sdsm_post_objects_multi, of which
 * only d_g -- here the smoothed glare image --, H, W and n_objects are read).  Per object: the fragment eroded by disk(2) with its
 * border as foreground; max and min of d_g over it; for each of the num_layers proportions h_props (HOST doubles) the layer
 * eroded & (d_g > (max - min) * prop + min), the threshold in two rounded operations.  d_out[2i] = pixels of the eroded mask,
 * d_out[2i+1] = bit l set iff layer l has more than one 4-connected component (all clear when a masked value is NaN).  d_out[2i] =
 * -1: the fragment exceeds 4096 words of whole-word rows and has no 3 * h * ceil(w / 32) words at d_ws + d_ws_off[i]; -2: its box is
 * empty or reaches outside its image.  1 <= num_layers <= SDSM_POST_MAX_GLARE_LAYERS. */
int sdsm_post_glare_multi(const sdsm_post_image *images, int n_images, const int32_t *d_boxes, const int64_t *d_bits_off,
                          const uint32_t *d_bits, const double *h_props, int num_layers, uint32_t *d_ws, const int64_t *d_ws_off,
                          int32_t *d_out, void *stream);
/* Separable Gaussian filter with SciPy's defaults (mode 'reflect', truncate 4): the smoothing of postprocess.py:165-166 and the
 * building block of sdsm_preprocess. */
size_t sdsm_gaussian_workspace_bytes(int H, int W, double sigma);
int sdsm_gaussian_filter(const double *d_in, int H, int W, double sigma, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
/* The same with caller-given SYMMETRIC weights per axis (HOST arrays of 2 R + 1 doubles): axis 0 with h_w0, then axis 1 with h_w1,
 * 'reflect' boundary -- e.g. the derivative-of-Gaussian filters of scipy.ndimage.gaussian_laplace used by the scale estimation
 * (superdsm/automation.py:52).  Radii up to R0 = 1240 and R1 = 10048 (the LDS tiles); longer filters fail before anything is launched. */
size_t sdsm_separable_workspace_bytes(int H, int W, int R0, int R1);
int sdsm_separable_filter(const double *d_in, int H, int W, const double *h_w0, int R0, const double *h_w1, int R1,
                          double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- scale estimation: determinant-of-Hessian blobs (superdsm/automation.py:13-68) ------------------------------
 * Bit for bit the host restatement of superdsm_amd/automation.py (_log_negative_masks, _integ, _hessian_matrix_det, _blob_doh).
 * Laplacian-of-Gaussian sign masks of n_scales scales in one call, without host synchronisation between them:
 * d_masks[s*H*W + p] = ((d2/dr2 + d2/dc2) im)[p] < 0 (uint8), each term two separable 'reflect' passes as in sdsm_separable_filter.
 * d_weights (DEVICE): per scale s, 2 R_s + 1 symmetric weights of order 0 and then 2 R_s + 1 of order 2, the scales one after
 * another; h_radii (host): R_s.  Radii as sdsm_separable_filter takes them. */
size_t sdsm_log_masks_workspace_bytes(int H, int W);
int sdsm_log_masks(const double *d_im, int H, int W, int n_scales, const int32_t *h_radii, const double *d_weights, uint8_t *d_masks,
                   void *d_workspace, size_t workspace_bytes, void *stream);
/* Integral image d_ii = im.cumsum(0).cumsum(1), every column and then every row summed in index order (numpy's rounding).
 * d_ii may be d_im. */
int sdsm_integral_image(const double *d_im, int H, int W, double *d_ii, void *stream);
/* The determinant-of-Hessian cube of all scales in one launch: d_cube[s*H*W + r*W + c] = mask_s[r, c] * det_s(r, c) with det_s
 * the box-filter determinant on the integral image d_ii.  h_box (host): n_scales x (size, s2, s3) int32 with size = int(3 sigma),
 * s2 = (size - 1) // 2, s3 = size // 3; h_w_i (host): n_scales doubles 1.0 / size / size.  d_masks as sdsm_log_masks writes them,
 * or NULL for none.  n_scales <= SDSM_DOH_MAX_SCALES. */
#define SDSM_DOH_MAX_SCALES 32
int sdsm_doh_cube(const double *d_ii, int H, int W, int n_scales, const int32_t *h_box, const double *h_w_i, const uint8_t *d_masks,
                  double *d_cube, void *stream);
/* Peaks of the cube: voxels equal to the maximum of their in-bounds 3x3x3 neighbourhood and > threshold.  d_out: a 16-byte header
 * (int64 total number of peaks, 8 bytes unused) followed by room for `capacity` records; the first min(total, capacity) peaks found
 * are written, in no particular order.  The total is exact whatever the capacity. */
typedef struct {
    int32_t r, c, s, reserved;
    double value;
} sdsm_doh_peak;
int sdsm_doh_peaks(const double *d_cube, int H, int W, int n_scales, double threshold, void *d_out, int64_t capacity, void *stream);

/* ---- coarse-to-fine region analysis (superdsm/c2freganal.py:110-126) ------------------------------------------------------------
 * sdsm_c2f_markers: the cluster markers of y (H x W float64): fg = y > 0, its 4-connected components numbered in raster order of
 * their first pixel (ndi.label), a component is irregular if (its pixels with an in-image 4-neighbour outside fg) / (its pixels)
 * > max_irregularity as a float64 division; background counts as one more component with irregularity 0.  d_y_mask (uint8): 0 on
 * irregular components; d_markers (int32): the regular components relabelled 1 .. n in raster order, 0 elsewhere -- all 0 if no pixel
 * is background (_normalize_labels_map(first_label=0) without label 0); d_count (device int32): n.  Byte-equal to the SciPy
 * statement.  H * W < 2^31. */
size_t sdsm_c2f_markers_workspace_bytes(int H, int W);
int sdsm_c2f_markers(const double *d_y, int H, int W, double max_irregularity, uint8_t *d_y_mask, int32_t *d_markers, int32_t *d_count,
                     void *d_ws, size_t ws_bytes, void *stream);
/* sdsm_edt_exact: d_out[p] (float64) = Euclidean distance of pixel p to the nearest pixel with d_target != 0, unbounded; the exact
 * integer squared distance, then a correctly rounded sqrt: bit-equal to ndi.distance_transform_edt(d_target == 0).  Without any
 * target, the distance to (-1, 0), as SciPy reports it.  H, W <= 65535. */
size_t sdsm_edt_exact_workspace_bytes(int H, int W);
int sdsm_edt_exact(const uint8_t *d_target, int H, int W, double *d_out, void *d_ws, size_t ws_bytes, void *stream);
/* sdsm_watershed (host, no device access): the marker flood of the restated rule.  image: H x W float64; markers:
 * int32 (0 = unlabelled); mask: uint8 or NULL (all admissible).  Markers inside the mask are pushed first, in raster order, with age 0;
 * the heap pops the smallest (image value, push age, raster index); a popped pixel labels its unlabelled admissible 4-neighbours (up,
 * left, right, down) with its own label and pushes them with the next age.  out: int32 labels, 0 outside the mask and where no marker
 * reaches. */
int sdsm_watershed(const double *image, const int32_t *markers, const uint8_t *mask, int H, int W, int32_t *out);

/* ---- image sets: the image-wide steps above for several images at once ----------------------------------------------------------
 * A *_multi entry point runs one step for a set of 1 .. SDSM_MAX_SET_IMAGES images: every kernel phase is ONE launch for the whole set,
 * with no host synchronisation between images (a caller splits larger sets).  The set is described by a HOST table of
 * sdsm_set_image: image i has H x W pixels (row-major) starting at element `offset` of every packed pixel buffer of the call (counted
 * in that buffer's element type).  Pixel indices stay local to their image, so only each image is bound by the single-image limits and
 * the set may hold more than 2^31 pixels.  The images must not overlap in an output buffer.  The table is read on the host; it
 * reaches the device with the launches, so the caller may free it when the call returns.  Per image, the results are byte-equal to
 * the single-image entry point, which is the set of one image {0, H, W}.  The workspace sizes grow with the set (adding an image never shrinks them); 0 = bad table. */
#define SDSM_MAX_SET_IMAGES 32
typedef struct {
    int64_t offset;         /* first element of the image in the packed buffers, >= 0 */
    int32_t H, W;           /* >= 1 */
} sdsm_set_image;
/* sdsm_c2f_markers for every image of the set (c2freganal.py:110-123): d_y (float64), d_y_mask (uint8) and d_markers (int32) packed as
 * the table says; max_irregularity: HOST array, one threshold per image; d_count (device): n_images int32, the markers of each image.
 * H * W < 2^31 per image. */
size_t sdsm_c2f_markers_workspace_bytes_multi(const sdsm_set_image *images, int n_images);
int sdsm_c2f_markers_multi(const sdsm_set_image *images, int n_images, const double *d_y, const double *max_irregularity, uint8_t *d_y_mask,
                           int32_t *d_markers, int32_t *d_count, void *d_ws, size_t ws_bytes, void *stream);
/* sdsm_edt_exact for every image of the set: d_target (uint8) and d_out (float64) packed as the table says.  H, W <= 65535 per image. */
size_t sdsm_edt_exact_workspace_bytes_multi(const sdsm_set_image *images, int n_images);
int sdsm_edt_exact_multi(const sdsm_set_image *images, int n_images, const uint8_t *d_target, double *d_out, void *d_ws, size_t ws_bytes,
                         void *stream);

/* ---- label maps and overlays of a result (superdsm/render.py:137-451) --------------------------------------------------------------
 * The kernel phases of render.rasterize_labels_gpu / render_result_over_image_gpu and their image-set forms; the definition they are
 * tested against is the host code of superdsm_amd/render.py.  Objects are given as sdsm_post_objects takes them: d_boxes n x 4 int32
 * (r0, c0, h, w, in the coordinates of the object's image), the h * w bits of the fragment row-major, LSB first in uint32 words at
 * d_bits + d_bits_off[i].  A *_multi form takes the set as a HOST table of sdsm_set_image (1 .. SDSM_MAX_SET_IMAGES images, H, W <=
 * 65535, H * W < 2^31) and the image of every object in d_obj_image (int32, may be NULL for one image); the pixel buffers are packed as
 * the table says.  The single-image form is the set of that one image: the same kernels, the same bytes.  Only integer atomics whose
 * result does not depend on the arrival order are used: a second launch gives the same bytes. */
#define SDSM_RENDER_MAX_RADIUS 16
/* render.py:380-384 (rasterize_objects): object i dilated (radius > 0) or eroded (radius < 0) by disk(|radius|), 1 <= |radius| <= 16,
 * in the window of its box grown by |radius| and clipped to the image (dilation: outside the image is background; erosion: outside
 * is foreground).  The window's bits go to d_new_bits + d_new_off[i] (in words, (window pixels + 31) / 32 words each), the number of
 * set pixels to d_area[i]. */
int sdsm_render_morph(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, int radius,
                      const int64_t *d_new_off, uint32_t *d_new_bits, int32_t *d_area, void *stream);
int sdsm_render_morph_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                            const int64_t *d_bits_off, const uint32_t *d_bits, int radius, const int64_t *d_new_off, uint32_t *d_new_bits,
                            int32_t *d_area, void *stream);
/* render.py:398-401 (rasterize_labels): d_inter[k] = |A n B| for the pair k of objects d_pairs[2 k], d_pairs[2 k + 1] of one image, an
 * exact integer; the division by the smaller area and the merge bookkeeping stay on the host.  Serves any number of images. */
int sdsm_render_overlaps(int n_pairs, const int32_t *d_pairs, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits,
                         int32_t *d_inter, void *stream);
/* render.py:425-431: d_obj_label[i] >= 1 is the label of the (merged) object that object i belongs to.  d_label (int32): the highest
 * label covering a pixel (the definition assigns the labels in ascending order), 0 where two different labels meet and on the
 * background; d_cover (uint8): 0 background, 1 one label, 2 several; d_target (uint8): d_label != 0, the input of sdsm_edt_exact.
 * All three are cleared by the call; n may be 0. */
int sdsm_render_paint(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits,
                      const int32_t *d_obj_label, int32_t *d_label, uint8_t *d_cover, uint8_t *d_target, void *stream);
int sdsm_render_paint_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                            const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label, int32_t *d_label,
                            uint8_t *d_cover, uint8_t *d_target, void *stream);
/* render.py:432-433: the pixels the flood can touch, per image: the pixels with d_cover == 2 (label 0) and the labelled pixels with such
 * a 4-neighbour, each as (raster index in its image, label, d_dist there).  Image i writes at most capacity[i] entries (HOST array)
 * behind those of the images before it, in no particular order; d_counts[i] is the exact number found. */
typedef struct {
    int32_t idx, label;
    double dist;
} sdsm_render_entry;
int sdsm_render_compact(int H, int W, const int32_t *d_label, const uint8_t *d_cover, const double *d_dist, int64_t capacity,
                        sdsm_render_entry *d_entries, int32_t *d_count, void *stream);
int sdsm_render_compact_multi(const sdsm_set_image *images, int n_images, const int32_t *d_label, const uint8_t *d_cover, const double *d_dist,
                              const int64_t *capacity, sdsm_render_entry *d_entries, int32_t *d_counts, void *stream);
/* sdsm_flood_sparse (host, no device access): the priority flood of superdsm_amd/render.py:_watershed (what render.py:433 asks of
 * skimage.segmentation.watershed) on the entries of one image, sorted by ascending idx: entries with label > 0 are seeds, pushed in
 * raster order with ages 0, 1, 2, ...; the heap pops the smallest (dist, age, row, column); a popped pixel gives its label to its
 * unlabelled neighbours in the set, visited up, down, left, right, which enter with the next ages.  out[k]: the label of entry k, 0
 * where no seed reaches.  This is not the rule of sdsm_watershed (all markers age 0; up, left, right, down). */
int sdsm_flood_sparse(int64_t n, const int32_t *idx, const int32_t *label, const double *dist, int H, int W, int32_t *out);
/* d_label[d_pix[k]] = d_lab[k] for n entries (d_pix: int64 elements into the packed buffer, distinct): the flood's labels. */
int sdsm_render_scatter(int64_t n, const int64_t *d_pix, const int32_t *d_lab, int32_t *d_label, void *stream);
/* render.py:443-447, exactly coinciding objects: d_lost[l] (n_labels + 1 int32) = the pixels of label l's objects that have d_label 0,
 * d_max[image] = the highest label in the image.  sdsm_render_fill: the pixels of the objects d_sel[0 .. n_sel) that have d_label 0 get
 * new_label (1 .. 65535); *d_filled = their number (> 0 iff any; pixels shared by two selected objects may count twice). */
int sdsm_render_lost(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label,
                     int n_labels, int32_t *d_label, int32_t *d_lost, int32_t *d_max, void *stream);
int sdsm_render_lost_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                           const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label, int n_labels, int32_t *d_label,
                           int32_t *d_lost, int32_t *d_max, void *stream);
int sdsm_render_fill(int H, int W, int n_sel, const int32_t *d_sel, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits,
                     const int32_t *d_obj_label, int new_label, int32_t *d_label, int32_t *d_filled, void *stream);
int sdsm_render_fill_multi(const sdsm_set_image *images, int n_images, int n_sel, const int32_t *d_sel, const int32_t *d_obj_image,
                           const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label,
                           int new_label, int32_t *d_label, int32_t *d_filled, void *stream);
/* render.py:449: d_out[p] (uint16) = d_label[p], or (uint16) background_label (-65535 .. 0; -1 reads 65535) where it is 0, for the n
 * elements of a packed buffer. */
int sdsm_render_finish(int64_t n, const int32_t *d_label, int background_label, uint16_t *d_out, void *stream);
/* The overlays (render.py:246-262 rasterize_regions, :265-287 render_regions_over_image, :291-365 render_result_over_image) in one
 * pass over the image.  With mn / mx the minimum / maximum of d_labels (int32, >= 0) over the in-image pixels of disk(radius), 0 <=
 * radius <= 16, around a pixel (a tile and its halo through LDS), a pixel is painted with color[0 .. 3) if
 *   kind 0 (regions):          mn != mx;  and blended bg[c] * bg[3] + v * (1 - bg[3]) if bg != NULL and mn == mx == background_label
 *   kind 1 (result, 'center'): mx > 0 and mn != mx
 *   kind 2 (result, 'inner'):  label > 0 and mn != mx          (the caller passes twice the contour's radius)
 *   kind 3 (rasterize_regions alone): nothing is painted; d_out holds ONE uint8 per pixel, bit 0 = mn != mx (border), bit 1 = bg !=
 *           NULL and mn == mx == background_label (only bg's presence is read); d_base, channels and color are ignored (may be NULL)
 * and keeps d_base (float64, channels = 1 or 3 per pixel) otherwise; d_out: 3 uint8 per pixel, 255 * v truncated (kind 0) or rounded
 * half to even (kinds 1, 2) and clipped to 0 .. 255.  color and bg (4 doubles, or NULL) are HOST arrays. */
int sdsm_render_overlay(int H, int W, const int32_t *d_labels, const double *d_base, int channels, int kind, int radius, const double *color,
                        const double *bg, int background_label, uint8_t *d_out, void *stream);
int sdsm_render_overlay_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const double *d_base, int channels,
                              int kind, int radius, const double *color, const double *bg, int background_label, uint8_t *d_out, void *stream);

/* ---- colour maps and adjacency graphs (superdsm/render.py:13-134, :454-508) --------------------------------------------------------
 * render_ymap, shuffle_labels / colorize_labels and draw_line / render_adjacencies; the definitions they are tested against are the
 * *_host functions of superdsm_amd/render.py.  Conventions as above: pixel buffers packed as the HOST table of sdsm_set_image says, the
 * single-image form is the set of that one image, integer atomics only (a second launch gives the same bytes).
 *
 * A colour map is a DEVICE table d_lut of (N + 3) x 4 float64, 1 <= N <= SDSM_RENDER_MAX_COLORS: the N colours, then the colours for
 * values below, above and "bad" (NaN), as matplotlib keeps them; the fourth column is not read.  The lookup of x is matplotlib's
 * Colormap.__call__ for float input: xa = x * N; xa == N reads N - 1; xa < 0 below; xa >= N above; NaN bad; else entry (int)xa. */
#define SDSM_RENDER_MAX_COLORS 1024
#define SDSM_RENDER_MAX_SEED_RADIUS 64
/* render.py:462-473 (shuffle_labels) and :503 (labels.min(), labels.max()): with a permutation table (d_perm != NULL; image i owns
 * d_perm[perm_off[i] .. perm_off[i + 1]), indexed by label - perm_min[i]; perm_off with n_images + 1 entries and perm_min are HOST
 * arrays) a label reads its table entry, a label outside its table reads 0 (render.py:469); without one the labels stay.  d_range (2
 * int32 per image, may be NULL) receives the minimum and maximum of the resulting labels, d_permuted (int32, packed as d_labels, may
 * be NULL) the resulting labels. */
int sdsm_render_label_range(int H, int W, const int32_t *d_labels, const int32_t *d_perm, int64_t perm_n, int perm_min, int32_t *d_range,
                            int32_t *d_permuted, void *stream);
int sdsm_render_label_range_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_perm,
                                  const int64_t *perm_off, const int32_t *perm_min, int32_t *d_range, int32_t *d_permuted, void *stream);
/* d_out: 3 float64 per pixel, the colour of
 *   source 0 (render.py:127-134, render_ymap): d_src float64; x = (min(max(y, lo), hi) - sub) / div with (lo, hi, sub, div) = the four
 *            doubles of image i in the HOST array clim, unfused, a NaN staying NaN.  d_flags[i] (int32, cleared by the call) gets bit
 *            0 if the image holds a NaN: numpy's y.min() is NaN then and EVERY pixel of the definition is "bad", which is for the
 *            caller to return.
 *   source 1 (render.py:503-507, colorize_labels): d_src int32 labels, permuted as sdsm_render_label_range does; x = (double)(label -
 *            min) / (double)(max - min) with (min, max) = d_range of the image (0 / 0 = NaN: "bad"); bg_color (3 HOST doubles) where
 *            bg_color != NULL and the label equals bg_label. */
int sdsm_render_colormap(int H, int W, int source, const void *d_src, const double *d_lut, int N, const double *clim, const int32_t *d_perm,
                         int64_t perm_n, int perm_min, const int32_t *d_range, const double *bg_color, int bg_label, int32_t *d_flags,
                         double *d_out, void *stream);
int sdsm_render_colormap_multi(const sdsm_set_image *images, int n_images, int source, const void *d_src, const double *d_lut, int N,
                               const double *clim, const int32_t *d_perm, const int64_t *perm_off, const int32_t *perm_min,
                               const int32_t *d_range, const double *bg_color, int bg_label, int32_t *d_flags, double *d_out, void *stream);
/* render.py:13-99 (draw_line, render_adjacencies).  d_prims: n_prims x 8 int32 (kind, index, image, r0, c0, r1, c1, 0); kind 0 is a
 * seed at (r0, c0), kind 1 the line number `index` (0 .. 65534, the list order) from (r0, c0) to (r1, c1).  Seeds and end points lie
 * INSIDE their image: the caller checks that.  Painted in the definition's order, whatever the order of d_prims:
 *   1. every seed's rim, the pixels with ((r - r0) / rim_radius)^2 + ((c - c0) / rim_radius)^2 < 1 (float64, as written: what
 *      skimage.draw.disk documents), colors[0 .. 3);
 *   2. the lines by ascending index.  A line's pixels are those of skimage.draw.line (integer Bresenham: the longer axis drives,
 *      columns on a tie; error term from 2 d_short - d_long; last pixel = the end point).  A pixel whose squared distance to the nearest
 *      line pixel is <= core_d2 gets colors[6 .. 9), else if <= ring_d2 colors[9 .. 12) (the ring of a fractional thickness,
 *      render.py:40-44; core_d2 = -1: no core); line_reach = floor(sqrt(ring_d2)) <= 16;
 *   3. every seed's disk (disk_radius), colors[3 .. 6).
 * Radii 0 .. SDSM_RENDER_MAX_SEED_RADIUS.  Unpainted pixels keep d_base (float64, channels = 1 or 3 per pixel).  d_out: 3 uint8 per
 * pixel, 255 * v clipped to 0 .. 255 and truncated (render.py:99).  d_key (int32 per pixel, packed) is scratch, cleared by the call:
 * the per-pixel integer maximum that makes the result independent of the arrival order.  colors: 12 HOST doubles. */
int sdsm_render_graph(int H, int W, int n_prims, const int32_t *d_prims, double rim_radius, double disk_radius, int line_reach, int core_d2,
                      int ring_d2, const double *colors, const double *d_base, int channels, int32_t *d_key, uint8_t *d_out, void *stream);
int sdsm_render_graph_multi(const sdsm_set_image *images, int n_images, int n_prims, const int32_t *d_prims, double rim_radius,
                            double disk_radius, int line_reach, int core_d2, int ring_d2, const double *colors, const double *d_base,
                            int channels, int32_t *d_key, uint8_t *d_out, void *stream);

/* ---- per-object measurement tables (no reference counterpart beyond tests/regression/validate.py:31-36 and the eccentricity of
 * superdsm/postprocess.py:340-344) ---------------------------------------------------------------------------------------------------
 * One record per object or per label: the exact integer sums from which superdsm_amd/measure.py derives counts, sizes, positions,
 * shapes and intensities on the host; the definitions the kernels are tested against are its *_host functions.  Conventions as
 * for the label maps: objects as sdsm_post_objects takes them, sets as a HOST table of sdsm_set_image (1 .. SDSM_MAX_SET_IMAGES images,
 * H, W <= 65535, H * W < 2^31), pixel buffers packed as the table says, the single-image form is the set of that one image.  Every sum
 * over pixels is an integer sum and every atomic an integer add / min / max / or: the bytes do not depend on the order, the launch or
 * the set size, and a second launch gives the same bytes.
 *
 * Ranges: r, c <= 65534 and area < 2^31, so sum_rr < 2^63 and nothing wraps.
 * Intensities (d_g, float64, optional): per image, e is the smallest exponent with (max finite |g|) < 2^e, clamped to -960 .. 1024, 0 for
 * an image without a non-zero finite pixel.  A finite pixel adds q = rint(ldexp(g, 62 - e)) as a signed 64-bit integer: its bits
 * 0 .. 31 to gsum_lo, the arithmetic shift q >> 32 to gsum_hi; the sum is (gsum_hi * 2^32 + gsum_lo) * 2^(e - 62), exact up to half a
 * quantum 2^(e - 62) per pixel.  A non-finite pixel sets flag bit 1 and adds nothing.  A first kernel leaves each image's max finite
 * |g| in d_gmax_abs (n_images float64) and the measuring kernels take e from there; d_scale_exp (n_images int32, may be NULL) receives
 * e.  Without d_g both may be NULL, the intensity fields are those of an object without a finite pixel and e is 0.  112 bytes. */
typedef struct {
    int64_t area;                       /* pixels */
    int64_t sum_r, sum_c;               /* sums of the row / column indices, image coordinates */
    uint64_t sum_rr, sum_rc, sum_cc;    /* sums of r * r, r * c, c * c */
    int32_t r0, c0, r1, c1;             /* bounding box of the pixels, end exclusive; all 0 when area == 0 */
    int32_t flags;                      /* bit 0: the box touches the image border; bit 1: a non-finite intensity inside */
    int32_t scale_exp;                  /* e of the record's image */
    int64_t n_finite;                   /* pixels with a finite intensity */
    uint64_t gsum_lo;                   /* low limb of the intensity sum */
    int64_t gsum_hi;                    /* high limb of the intensity sum */
    double gmin, gmax;                  /* over the finite pixels (-0.0 reads +0.0); +inf / -inf when there are none */
} sdsm_measure_record;
/* One record per object (one workgroup each, no global atomics): d_out[i] for object i of d_boxes / d_bits_off (n of them; d_obj_image
 * int32, NULL for one image).  Objects may overlap.  The bits of a fragment's last word past h * w are ignored; a fragment without a set
 * bit, and an object whose box is empty or leaves its image, give the zero record (all integers 0 but scale_exp; gmin, gmax +inf, -inf). */
int sdsm_measure_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                         double *d_gmax_abs, int32_t *d_scale_exp, sdsm_measure_record *d_out, void *stream);
int sdsm_measure_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                               const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                               sdsm_measure_record *d_out, void *stream);
/* One record per label of a label map (d_labels int32, packed): image i owns the records rec_off[i] + label of d_out for the labels
 * 0 .. n_labels[i] - 1 (rec_off, n_labels: HOST arrays; 1 <= n_labels <= SDSM_MEASURE_MAX_LABELS; the ranges must not overlap).  The
 * call clears them; an absent label keeps the zero record.  A label outside 0 .. n_labels[i] - 1 is counted in d_bad[i] (int32 per
 * image, cleared by the call) and skipped. */
#define SDSM_MEASURE_MAX_LABELS 65536
int sdsm_measure_labels(int H, int W, const int32_t *d_labels, int n_labels, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                        sdsm_measure_record *d_out, int32_t *d_bad, void *stream);
int sdsm_measure_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off,
                              const int32_t *n_labels, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                              sdsm_measure_record *d_out, int32_t *d_bad, void *stream);

/* ---- contour shape tables (no reference counterpart; the definitions are shape_objects_host and shape_labels_host of
 * superdsm_amd/shape.py) --------------------------------------------------------------------------------------------------------------
 * One record of exact integers per object, from which superdsm_amd/shape.py derives perimeter, circularity, convex area, solidity and
 * the Feret diameters on the host, and the vertices of its convex hull.  An object is the set P of the set bits of its fragment;
 * everything else -- the rest of its box, other objects, the outside of the image -- is outside P (unlike the boundary distances below,
 * where the image frame makes no boundary).  Conventions as for the measurement tables: objects as sdsm_post_objects takes them, sets
 * as a HOST table of sdsm_set_image (H, W <= 65535, H * W < 2^31), the single-image form is the set of that one image; every count is an
 * integer sum and every atomic an integer add / min / max / or, so the bytes do not depend on the order, the launch or the set size.
 *
 * border pixel: a pixel of P with a 4-neighbour outside P.  For a border pixel, v = 1 + 2 * (border pixels among its 4 orthogonal
 * neighbours) + 10 * (border pixels among its 4 diagonal neighbours); perim_n1 counts v in {5, 7, 15, 17, 25, 27}, perim_n2 v in
 * {21, 33}, perim_n3 v in {13, 23}: the classes of the 4-neighbourhood perimeter estimator n1 + n2 * sqrt(2) + n3 * (1 + sqrt(2)) / 2.
 * Hull: of the corners of the closed unit squares of the pixels, on the lattice 0 .. H x 0 .. W; vertices (row, column) counter-clockwise
 * in the (row, column) plane from the smallest (row, column), collinear points dropped.  80 bytes. */
#define SDSM_SHAPE_MAX_CHAIN 4096       /* vertices of the left or the right chain of a hull that the kernel holds (see DESIGN.md "Limits") */
#define SDSM_SHAPE_MAX_WINDOW_WORDS (1ll << 26)     /* label form: 32-bit words of all label windows of a call (256 MB) */
typedef struct {
    int64_t area;                       /* pixels of P */
    int64_t border_pixels;              /* border pixels */
    int64_t edges_r, edges_c;           /* unit edges between a pixel of P and an outside pixel above or below / left or right of it */
    int64_t perim_n1, perim_n2, perim_n3;
    int64_t hull_area2;                 /* twice the area of the hull (shoelace) */
    int64_t feret_max_d2;               /* largest squared distance between two hull vertices */
    int32_t n_vertices;                 /* hull vertices */
    int32_t flags;                      /* bit 0: the bounding box of P touches the image frame; bit 30: a hull chain passed
                                           SDSM_SHAPE_MAX_CHAIN vertices (the hull fields and vertices are then not valid) */
} sdsm_shape_record;
/* Host helper (no device access): the vertex slots an object with an h x w box needs in d_slots, 2 * min(h + 1, 2 * w + 2); 0 for an
 * empty box. */
int64_t sdsm_shape_vertex_slots(int h, int w);
/* d_out[i] for object i of d_boxes / d_bits_off (n of them; d_obj_image int32, NULL for one image), one workgroup each.  The bits of a
 * fragment past h * w are ignored, a box larger than the tight box changes nothing; a fragment without a set bit, and an object whose box
 * is empty or leaves its image, give the zero record and no vertex.  Hull vertices: object i writes (row, column) int32 pairs, image
 * coordinates, from pair d_slot_off[i] (int64) of d_slots on, sdsm_shape_vertex_slots(h, w) pairs at most (workspace of the caller);
 * then d_vert_off (n + 1 int64) receives the exclusive sum of n_vertices and d_verts the vertices of all objects one behind the other
 * (d_vert_off[n] pairs; room for as many pairs as d_slots holds is enough). */
int sdsm_shape_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_slot_off,
                       int32_t *d_slots, sdsm_shape_record *d_out, int64_t *d_vert_off, int32_t *d_verts, void *stream);
int sdsm_shape_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                             const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_slot_off, int32_t *d_slots,
                             sdsm_shape_record *d_out, int64_t *d_vert_off, int32_t *d_verts, void *stream);
/* The same for labels of label maps (d_labels int32, packed): the caller names n windows (d_obj_image, d_boxes, d_bits_off into the
 * workspace d_bits of window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS words, which the call clears) and, per image, the window of every label:
 * d_label_obj[rec_off[i] + l] is the window of label l of image i, or negative for a label that is not measured (rec_off, n_labels: HOST
 * arrays as for sdsm_measure_labels, whose records give the boxes).  A first kernel sets the bit of every pixel in the window of its
 * label -- a pixel of another label stays outside --, then the windows are measured as objects.  A pixel outside the box of its label's
 * window is skipped; a label outside 0 .. n_labels[i] - 1 is counted in d_bad[i] (int32 per image, cleared by the call) and skipped. */
int sdsm_shape_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                      const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const int64_t *d_slot_off, int32_t *d_slots,
                      sdsm_shape_record *d_out, int64_t *d_vert_off, int32_t *d_verts, int32_t *d_bad, void *stream);
int sdsm_shape_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                            const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                            int64_t window_words, uint32_t *d_bits, const int64_t *d_slot_off, int32_t *d_slots, sdsm_shape_record *d_out,
                            int64_t *d_vert_off, int32_t *d_verts, int32_t *d_bad, void *stream);

/* ---- intensity distribution tables (no reference counterpart; the definitions are intensity_objects_host and intensity_labels_host of
 * superdsm_amd/intensity.py) ----------------------------------------------------------------------------------------------------------
 * Per object, over the FINITE intensities of its pixels (d_g, float64, required; a non-finite pixel sets flag bit 1 and is counted
 * out): extremes, an exact spread centred on the object's own minimum, exact order statistics for up to SDSM_INTENSITY_MAX_QUANTILES
 * quantiles, and the two middle order statistics of |g - median|.  superdsm_amd/intensity.py derives standard deviation, mean,
 * median, quantiles, interquartile range and median absolute deviation on the host.  Conventions as for the measurement tables (objects
 * as sdsm_post_objects takes them, sets as a HOST table of sdsm_set_image, H, W <= 65535, H * W < 2^31); every sum is an integer sum and
 * every order statistic an element of the input, so the bytes do not depend on the order, the launch or the set size.  -0.0 reads +0.0
 * everywhere.
 *
 * Spread: d = gmax - gmin (one IEEE subtraction); range_exp e is the smallest exponent with d < 2^e, clamped to -960 .. 1024, 0 when
 * d == 0.  A finite pixel adds p = rint(ldexp(g - gmin, 30 - e)) (one IEEE subtraction, ties to even; 0 <= p <= 2^30): p to sum_p, bits
 * 0 .. 31 of p * p to sum_pp_lo, p * p >> 32 to sum_pp_hi.  With S2 = sum_pp_hi * 2^32 + sum_pp_lo the variance is
 * (n_finite * S2 - sum_p^2) / n_finite^2 * 4^(e - 30); its root is within 2^(e - 30) of the population standard deviation of the doubles.
 * If d is not finite (gmin and gmax further apart than the largest double), flag bit 3 is set, range_exp is 1024 and the three sums
 * stay 0.
 * Order statistics: quantile q = num[q] / den[q] (HOST arrays, launch arguments; 0 <= num <= den, 1 <= den <= SDSM_INTENSITY_MAX_DEN)
 * of an object with n = n_finite >= 1 has the ranks of sdsm_quantile_ranks; d_order[(i * n_q + q) * 2 + 0 / 1] receive the elements at
 * the ranks lo / hi of the sorted finite intensities, bit for bit.  With n == 0 both hold the quiet NaN 0x7ff8000000000000.
 * MAD: med_lo, med_hi are the order statistics at the ranks of 1 / 2, whatever the caller's quantiles, and med = 0.5 * med_lo + 0.5 *
 * med_hi (two products, one sum, no fused multiply-add); mad_lo, mad_hi are the order statistics at those ranks of the keys |g - med|
 * (one IEEE subtraction each; +inf where it overflows); all four NaN with n == 0.
 * Objects with at most SDSM_INTENSITY_LDS_KEYS finite pixels are selected from a copy in LDS; larger ones re-read their pixels in every
 * round of the selection: the same bytes, more slowly (see DESIGN.md "Limits").  96 bytes. */
#define SDSM_INTENSITY_MAX_QUANTILES 8
#define SDSM_INTENSITY_MAX_DEN 1000000  /* largest denominator of a quantile */
#define SDSM_INTENSITY_LDS_KEYS 4096    /* finite pixels of an object whose keys are staged in LDS (32 KB) */
typedef struct {
    int64_t area;                       /* pixels */
    int64_t n_finite;                   /* pixels with a finite intensity */
    int64_t sum_p;                      /* sum of p, < 2^61 */
    uint64_t sum_pp_lo, sum_pp_hi;      /* sums of the low 32 bits and of the rest of p * p, each < 2^63 */
    double gmin, gmax;                  /* over the finite pixels; +inf / -inf when there are none */
    double med_lo, med_hi;              /* the two middle order statistics of g (the ranks of 1 / 2); quiet NaN without a finite pixel */
    double mad_lo, mad_hi;              /* the two middle order statistics of |g - med|; quiet NaN without a finite pixel */
    int32_t range_exp;                  /* e */
    int32_t flags;                      /* bit 0: the bounding box of the pixels touches the image frame; bit 1: a non-finite intensity
                                           inside; bit 2: no finite pixel; bit 3: gmax - gmin is not finite */
} sdsm_intensity_record;
/* Host helper (no device access): the ranks of the quantile num / den of n sorted values, 1 <= n < 2^31: h = (n - 1) * num, lo = h div
 * den, rem = h mod den, hi = lo + (rem != 0).  The quantile is v[lo] + (v[hi] - v[lo]) * rem / den.  The kernels use the same inline
 * function. */
int sdsm_quantile_ranks(int64_t n, int32_t num, int32_t den, int64_t *lo, int64_t *hi, int64_t *rem);
/* d_out[i] and d_order[(i * n_q + q) * 2 ..] for object i of d_boxes / d_bits_off (n of them; d_obj_image int32, NULL for one image), one
 * workgroup each, no global atomics; neither output needs clearing.  0 <= n_q <= SDSM_INTENSITY_MAX_QUANTILES (d_order may be NULL for
 * n_q == 0).  The bits of a fragment past h * w are ignored, a box larger than the tight box changes nothing.  A fragment without a set
 * bit, and an object whose box is empty or leaves its image, give the empty record (integers 0, flags bit 2 alone, gmin, gmax +inf, -inf,
 * med_lo .. mad_hi NaN) and NaN slots.  n == 0: no launch. */
int sdsm_intensity_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                           int n_q, const int32_t *num, const int32_t *den, sdsm_intensity_record *d_out, double *d_order, void *stream);
int sdsm_intensity_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                 const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, int n_q, const int32_t *num,
                                 const int32_t *den, sdsm_intensity_record *d_out, double *d_order, void *stream);
/* The same for labels of label maps, by the windows of sdsm_shape_labels: the caller names n windows (d_obj_image, d_boxes, d_bits_off
 * into the workspace d_bits of window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS words, which the call clears) and d_label_obj; a first kernel
 * sets the bit of every pixel in the window of its label, then the windows are measured as objects.  d_bad as there. */
int sdsm_intensity_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                          const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int n_q, const int32_t *num,
                          const int32_t *den, sdsm_intensity_record *d_out, double *d_order, int32_t *d_bad, void *stream);
int sdsm_intensity_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off,
                                const int32_t *n_labels, const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int n_q,
                                const int32_t *num, const int32_t *den, sdsm_intensity_record *d_out, double *d_order, int32_t *d_bad,
                                void *stream);

/* ---- texture tables: grey-level co-occurrence per object (no reference counterpart; the definitions are texture_objects_host and
 * texture_labels_host of superdsm_amd/texture.py) --------------------------------------------------------------------------------------
 * Per object and offset the non-zero cells of the grey-level co-occurrence matrix as exact integer counts, from which
 * superdsm_amd/texture.py derives the Haralick features on the host.  Conventions as for the intensity tables (objects as
 * sdsm_post_objects takes them, sets as a HOST table of sdsm_set_image, H, W <= 65535, H * W < 2^31; d_g float64, required).
 *
 * Levels: image i has levels - 1 edges, d_edges[i * (levels - 1) ..] (float64 on the device, finite and strictly increasing: the
 * caller's duty, the device cannot be checked from here); the level of a finite pixel g is the number of edges <= g
 * (sdsm_texture_level), 0 .. levels - 1; -0.0 compares as 0.0.  A non-finite pixel has no level, takes part in no pair and sets flag
 * bit 1.  1 <= levels <= SDSM_TEXTURE_MAX_LEVELS; with levels == 1 d_edges may be NULL.
 * Offsets: n_offsets pairs (d_row, d_col) (HOST array, launch arguments), 1 <= n_offsets <= SDSM_TEXTURE_MAX_OFFSETS, none (0, 0), each
 * with max(|d_row|, |d_col|) <= SDSM_TEXTURE_MAX_REACH, none twice and none together with its negative.
 * Counts: for object k and offset o every pixel p with p and p + o both in the object and both finite adds 1 to the cell
 * (min(a, b), max(a, b)) of the levels a of p and b of p + o: the UNORDERED counts c(i, j), i <= j, each below 2^31.  The symmetric
 * matrix of the literature is c(i, j) off the diagonal and 2 c(i, i) on it.  Every count is an integer sum, and the cells are written in
 * ascending (i, j) order by a scan, so the bytes do not depend on the order, the launch or the set size. */
#define SDSM_TEXTURE_MAX_LEVELS 256
#define SDSM_TEXTURE_MAX_OFFSETS 8
#define SDSM_TEXTURE_MAX_REACH 32
#define SDSM_TEXTURE_MAX_SLOTS (1ll << 26)      /* entries of the padded list of a call, all objects and offsets (512 MB) */
typedef struct {
    int64_t area;                       /* pixels */
    int64_t n_finite;                   /* pixels with a finite intensity */
    int32_t level_min, level_max;       /* over the finite pixels; levels and -1 when there are none */
    int32_t flags;                      /* bit 0: the bounding box of the pixels touches the image frame; bit 1: a non-finite intensity
                                           inside; bit 2: no finite pixel */
    int32_t reserved;                   /* 0 */
} sdsm_texture_record;                  /* 32 bytes */
typedef struct {
    int64_t n_pairs;                    /* pairs of (object, offset): the sum of its counts */
    int64_t first;                      /* its first entry in d_entries: the running sum of n_entries */
    int32_t n_entries;                  /* its non-zero cells */
    int32_t reserved;                   /* 0 */
} sdsm_texture_pairs;                   /* 24 bytes */
typedef struct {
    uint16_t i, j;                      /* the cell, i <= j */
    uint32_t count;                     /* c(i, j) > 0 */
} sdsm_texture_entry;                   /* 8 bytes */
/* Host helpers (no device access), the inline functions the kernels use (csrc/sdsm_texture.h).  sdsm_texture_level: the level of g among
 * n_edges edges, -1 for a bad argument (n_edges outside 0 .. 255, edges NULL with n_edges > 0) or a non-finite g.  sdsm_texture_cell: the
 * place of the cell (i, j), 0 <= i <= j < levels, in the packed upper triangle, i * (2 levels - i + 1) / 2 + j - i; -1 otherwise. */
int sdsm_texture_level(const double *edges, int n_edges, double g);
int sdsm_texture_cell(int levels, int i, int j);
/* d_out[k] (n records), d_pairs[k * n_offsets + o] and the entries for object k of d_boxes / d_bits_off (n of them; d_obj_image int32,
 * NULL for one image), one workgroup per object and offset, no global atomics; no output needs clearing.  (k, o) writes its cells in
 * ascending (i, j) order into d_slots from entry d_slot_off[k * n_offsets + o] on, d_slot_off[k * n_offsets + o + 1] -
 * d_slot_off[k * n_offsets + o] at most (n * n_offsets + 1 int64, ascending, workspace of the caller; min(h * w, levels * (levels + 1) /
 * 2) entries are always enough; d_slot_off[n * n_offsets] <= SDSM_TEXTURE_MAX_SLOTS is the caller's to check); then `first` receives the
 * exclusive sum of n_entries and d_entries the cells of all (k, o) one behind the other (room for as many entries as d_slots holds is
 * enough).  The bits of a fragment past h * w are ignored, a box larger than the tight box changes nothing; nothing outside the box is
 * read.  A fragment without a set bit, and an object whose box is empty or leaves its image, give the empty record (integers 0,
 * level_min = levels, level_max = -1, flags bit 2 alone) and no pair.  n == 0: no launch. */
int sdsm_texture_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                         int levels, const double *d_edges, int n_offsets, const int32_t *offsets, const int64_t *d_slot_off,
                         sdsm_texture_entry *d_slots, sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs, sdsm_texture_entry *d_entries,
                         void *stream);
int sdsm_texture_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                               const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, int levels, const double *d_edges,
                               int n_offsets, const int32_t *offsets, const int64_t *d_slot_off, sdsm_texture_entry *d_slots,
                               sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs, sdsm_texture_entry *d_entries, void *stream);
/* The same for labels of label maps, by the windows of sdsm_shape_labels: the caller names n windows (d_obj_image, d_boxes, d_bits_off
 * into the workspace d_bits of window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS words, which the call clears) and d_label_obj; a first kernel
 * sets the bit of every pixel in the window of its label -- so a pair across two labels is not counted --, then the windows are measured
 * as objects.  d_bad as there. */
int sdsm_texture_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                        const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int levels, const double *d_edges,
                        int n_offsets, const int32_t *offsets, const int64_t *d_slot_off, sdsm_texture_entry *d_slots,
                        sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs, sdsm_texture_entry *d_entries, int32_t *d_bad, void *stream);
int sdsm_texture_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off,
                              const int32_t *n_labels, const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                              const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int levels,
                              const double *d_edges, int n_offsets, const int32_t *offsets, const int64_t *d_slot_off,
                              sdsm_texture_entry *d_slots, sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs,
                              sdsm_texture_entry *d_entries, int32_t *d_bad, void *stream);

/* ---- contingency table of two label maps (no reference counterpart; the definition is overlap_pairs_host of superdsm_amd/compare.py) --
 * For two label maps of one image (d_a, d_b: int32, packed as the table of the set says) the number of pixels of every pair of labels
 * (a, b) that occurs, background members included, in a hash table per image: image i owns the slots table_off[i] .. table_off[i] +
 * capacity[i] - 1 of d_keys and d_counts (table_off, capacity: HOST arrays; capacity a power of two >= 1; the ranges must not
 * overlap).  The call clears them on the stream.  An occupied slot holds the key (uint64_t)a << 32 | b and the 64-bit count of its
 * pixels; a free one the key ~0 and the count 0.  The order of the slots is that of the hash; after a sort by key the result does not
 * depend on the arrival order, the launch or the set size: every atomic is an integer compare-and-swap or add.
 * d_status: 2 int32 per image, cleared by the call.  [0]: pixels where either label is negative; they are skipped.  [1]: insertions
 * that found every slot of the table taken; their pixels are dropped, so the table is then incomplete (every count a lower bound) and
 * the caller launches again with a larger one.  The kernel never waits for a slot.  A table of >= H * W slots cannot fill up.
 * Limits: labels 0 .. 2^31 - 1, H * W < 2^31 per image (no limit per side: no coordinates are involved), 1 .. SDSM_MAX_SET_IMAGES
 * images. */
int sdsm_overlap_pairs_multi(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b,
                             const int64_t *table_off, const int64_t *capacity, uint64_t *d_keys, uint64_t *d_counts,
                             int32_t *d_status /* per image: [0] pixels with a negative label, [1] pairs without a slot */, void *stream);
int sdsm_overlap_pairs(int H, int W, const int32_t *d_a, const int32_t *d_b, int64_t capacity, uint64_t *d_keys,
                       uint64_t *d_counts, int32_t *d_status, void *stream);   /* the set of one image */

/* ---- boundary distances between two label maps (no reference counterpart; the definitions are label_boundaries_host and
 * pair_distances_host of superdsm_amd/boundary.py) -----------------------------------------------------------------------------------
 * A pixel of label l != 0 is a boundary pixel of l iff one of its 4-neighbours inside the image carries another label (the image border
 * makes no boundary).  For a pair of labels (a of map A, b of map B) the record below holds, in integers only, what the Hausdorff
 * distance, the mean surface distance and the normalised sum of distances follow from.  q(d2) = floor(sqrt(d2 * 2^32)) is the distance
 * in units of 2^-16 pixel, the exact integer root.  Conventions as for the measurement tables: sets as a HOST table of sdsm_set_image,
 * pixel buffers packed as the table says, the single-image form is the set of that one image; every atomic is an integer add or max,
 * so the records do not depend on the order, the launch, the set size or the work split, and no output buffer needs clearing.
 * Limits: labels 0 .. SDSM_BOUNDARY_MAX_LABELS - 1 (others are counted and skipped), H * H + W * W < 2^31 per image: every squared
 * distance fits int32, every side 16 bits and H * W < 2^30.  64 bytes. */
#define SDSM_BOUNDARY_MAX_LABELS 65536
#define SDSM_BOUNDARY_TILE 1024         /* boundary pixels of the target that a workgroup stages through LDS at a time */
#define SDSM_BOUNDARY_CHUNK 1024        /* query pixels of one work item (one workgroup) */
typedef struct {
    int32_t a, b;                       /* the two labels */
    int32_t boundary_a, boundary_b;     /* boundary pixels of each */
    int32_t max_d2_ab, max_d2_ba;       /* max over the boundary pixels of one of the min squared distance to the boundary of the other; -1 with a flag */
    int32_t flags;                      /* bit 0: the boundary of a is empty (also: a does not occur); bit 1: the same for b */
    int32_t reserved;                   /* 0 */
    int64_t sum_q_ab, sum_q_ba;         /* sums of q(min d2) over the same pixels as the maxima; 0 with a flag */
    int64_t nsd_num;                    /* sum over the pixels in exactly one of the two objects of q(min d2 to the boundary of b) */
    int64_t nsd_den;                    /* the same sum over the pixels in either object */
} sdsm_pair_distance;
/* One pass over a label map (d_labels int32, packed): image i owns the 2 * SDSM_BOUNDARY_MAX_LABELS int32 of d_counts from
 * i * 2 * SDSM_BOUNDARY_MAX_LABELS on: [2 l] the pixels of label l, [2 l + 1] its boundary pixels (0 for l = 0).  d_bad[i] (int32): the
 * pixels with a label outside the range; they are skipped.  Both are cleared by the call. */
int sdsm_label_pixel_counts_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int32_t *d_counts, int32_t *d_bad,
                                  void *stream);
int sdsm_label_pixel_counts(int H, int W, const int32_t *d_labels, int32_t *d_counts, int32_t *d_bad, void *stream);
/* The pixels of every label l >= 1 as one list per image, from the d_counts of the same map: d_start (SDSM_BOUNDARY_MAX_LABELS int32 per
 * image, written here) = the first entry of label l (the ranges of the labels are disjoint and dense, in no particular order); label l owns the
 * entries d_start[l] .. d_start[l] + pixels - 1 of the image's part of d_list (uint32, packed as the pixel buffers): its boundary pixels
 * first, then the others, each as row << 16 | column.  The order inside either part is the arrival order: sort before relying on it.
 * d_cursor (2 * SDSM_BOUNDARY_MAX_LABELS int32 per image) is scratch.  Entries of d_list that no label owns are not written. */
int sdsm_label_pixel_lists_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_counts, int32_t *d_start,
                                 int32_t *d_cursor, uint32_t *d_list, void *stream);
int sdsm_label_pixel_lists(int H, int W, const int32_t *d_labels, const int32_t *d_counts, int32_t *d_start, int32_t *d_cursor, uint32_t *d_list,
                           void *stream);
/* d_records[k] for the n_pairs pairs of d_pairs (4 int32 each: image, label a, label b, 0), from the counts, starts and lists of the two
 * maps d_a, d_b of the set.  The call initialises every record (a pair whose image or labels are out of range gets both flags).  The
 * work is the list d_items (n_items x 4 int32: pair, phase, chunk, 0), one workgroup each: phase 0 takes the boundary pixels of a
 * against the boundary of b (max_d2_ab, sum_q_ab), phase 1 those of b against the boundary of a, phase 2 all pixels of a and phase 3
 * the pixels of b that do not carry a in d_a, both against the boundary of b (nsd_num, nsd_den); chunk c stands for the entries
 * c * SDSM_BOUNDARY_CHUNK .. of that phase's pixel list.  A complete list names every chunk of every phase of every pair without a flag
 * once; an item of a flagged pair, out of range or past the end of its list does nothing.  n_pairs or n_items 0: no launch. */
int sdsm_pair_distances_multi(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b, const int32_t *d_counts_a,
                              const int32_t *d_counts_b, const int32_t *d_start_a, const int32_t *d_start_b, const uint32_t *d_list_a,
                              const uint32_t *d_list_b, int n_pairs, const int32_t *d_pairs, int64_t n_items, const int32_t *d_items,
                              sdsm_pair_distance *d_records, void *stream);
int sdsm_pair_distances(int H, int W, const int32_t *d_a, const int32_t *d_b, const int32_t *d_counts_a, const int32_t *d_counts_b,
                        const int32_t *d_start_a, const int32_t *d_start_b, const uint32_t *d_list_a, const uint32_t *d_list_b, int n_pairs,
                        const int32_t *d_pairs, int64_t n_items, const int32_t *d_items, sdsm_pair_distance *d_records, void *stream);
/* Host helper (no device access): out[k] = q(d2[k]) by the code the kernel runs (a float estimate, then a correction in 64-bit integers
 * until r * r <= d2 * 2^32 < (r + 1) * (r + 1)); a negative d2 gives 0. */
int sdsm_quantised_distance(const int32_t *d2, int64_t n, int64_t *out);

/* ---- neighbourhood tables of one label map (no reference counterpart; the definitions are neighbour_pairs_host and
 * neighbour_labels_host of superdsm_amd/neighbours.py) -------------------------------------------------------------------------------
 * How the objects of one label map lie to each other, in integers only.  Two pixels are WITHIN REACH iff their squared Euclidean
 * distance is <= max_d2, 1 <= max_d2 <= SDSM_NEIGHBOUR_MAX_D2 (a reach of 64 pixels; 1 sees edge contacts only, 2 the 8-connected ones).
 * Pairs: an unordered pair of labels a < b, both >= 1, has an entry iff some pixel of a and some pixel of b are within reach; min_d2 is
 * the smallest squared distance between a pixel of a and a pixel of b, contact_edges the number of crack edges between them (4-adjacent
 * pixel pairs with one pixel in each, counted once).  Labels: per label the pixels, the boundary pixels as sdsm_label_pixel_counts
 * defines them (the image frame makes no boundary), the boundary pixels with a pixel of another label >= 1 within reach, and the pixel
 * sides by what they face.  Label 0's record holds its area and zeros.
 * Conventions as for the tables above: sets as a HOST table of sdsm_set_image, d_labels int32 packed as the table says, the
 * single-image form is the set of that one image; every atomic is an integer min, add or compare-and-swap, so after a sort of the pair
 * table by key the bytes do not depend on the arrival order, the launch, the set size or the capacity.
 * Limits: labels 0 .. n_labels - 1 <= 65535 (others are counted and skipped: they count for nothing of their own and the other pixels
 * see them as label 0), H * H + W * W < 2^31 per image, 1 .. SDSM_MAX_SET_IMAGES images. */
#define SDSM_NEIGHBOUR_MAX_D2 4096
typedef struct {
    int64_t edges_background;           /* pixel sides of the label that face label 0 */
    int64_t edges_labels;               /* ... that face another label >= 1: the sum of contact_edges over the label's pairs */
    int64_t edges_frame;                /* ... that lie on the image frame */
    int32_t area;                       /* pixels */
    int32_t boundary;                   /* boundary pixels */
    int32_t close;                      /* boundary pixels with a pixel of another label >= 1 within reach; <= boundary */
    int32_t reserved;                   /* 0 */
} sdsm_neighbour_label;                 /* 40 bytes */
typedef struct {
    int32_t a, b;                       /* the two labels, 1 <= a < b */
    int32_t min_d2;                     /* 1 .. max_d2 */
    int32_t contact_edges;              /* > 0 iff min_d2 == 1 */
} sdsm_neighbour_pair;                  /* 16 bytes: a row of the sorted table the host makes of the occupied slots */
/* Host helpers (no device access), the inline functions the kernel uses (csrc/sdsm_neighbours.h).  sdsm_neighbour_halfwidth: the largest
 * |d_col| with d_row^2 + d_col^2 <= max_d2, by an integer root; -1 when the row lies outside the disk or max_d2 is outside
 * 1 .. SDSM_NEIGHBOUR_MAX_D2.  sdsm_neighbour_slot: the slot a key is tried at first in a table of `capacity` slots (linear probing
 * from there); -1 unless capacity is a power of two >= 1. */
int sdsm_neighbour_halfwidth(int max_d2, int d_row);
int64_t sdsm_neighbour_slot(uint64_t key, int64_t capacity);
/* d_label_out[rec_off[i] + l] for the labels 0 <= l < n_labels[i] of image i (rec_off, n_labels: HOST arrays, as
 * sdsm_measure_labels_multi takes them; 1 <= n_labels <= 65536; the ranges must not overlap), and the pairs of image i in the slots
 * table_off[i] .. table_off[i] + capacity[i] - 1 of d_keys, d_min_d2 and d_contact (HOST arrays; the per-image open-addressing table of
 * sdsm_overlap_pairs_multi with two uint32 values instead of one count): an occupied slot holds the key (uint64_t)a << 32 | b, a < b,
 * with its min_d2 and contact_edges; a free one the key ~0, min_d2 0xffffffff and contact_edges 0.  The call clears everything it
 * writes into, on the stream.
 * d_status: 2 int32 per image.  [0]: pixels with a label < 0 or >= n_labels; they are skipped.  [1]: insertions that found every slot
 * of the table taken; they are dropped, so the table is then incomplete and the caller launches again with a larger one (the label
 * records are complete all the same).  The kernel never waits for a slot. */
int sdsm_neighbours_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, const int64_t *rec_off,
                          const int32_t *n_labels, sdsm_neighbour_label *d_label_out, const int64_t *table_off, const int64_t *capacity,
                          uint64_t *d_keys, uint32_t *d_min_d2, uint32_t *d_contact, int32_t *d_status, void *stream);
int sdsm_neighbours(int H, int W, const int32_t *d_labels, int max_d2, int n_labels, sdsm_neighbour_label *d_label_out, int64_t capacity,
                    uint64_t *d_keys, uint32_t *d_min_d2, uint32_t *d_contact, int32_t *d_status, void *stream);   /* the set of one image */

/* ---- zone label maps of one label map (no reference counterpart; the definitions are nearest_other_host and zone_maps_host of
 * superdsm_amd/zones.py) ---------------------------------------------------------------------------------------------------------------
 * New label maps out of one label map, in integers only.  The map L (labels 0 .. 65535, 0 the background) is extended by label 0
 * outside the image frame.  NEAREST OTHER: for a pixel p, among the lattice places q with 0 < |p - q|^2 <= max_d2 and L(q) != L(p) the
 * one with the smallest key (|p - q|^2, L(q)) gives d2(p) and other(p); where there is none both are 0.  1 <= max_d2 <= SDSM_ZONE_MAX_D2
 * (a reach of 64 pixels).  So for a background pixel `other` is the nearest label >= 1 (the frame never counts), and for a pixel of a
 * label >= 1 d2 is its squared depth in the convention of the depth tables and `other` what it faces, 0 for background or frame.
 * ZONES: with depth(p) = d2(p), or SDSM_ZONE_NO_UPPER where nothing was found, a pixel is IN zone z iff lo_d2 < depth(p) <= hi_d2.  A
 * zone of side SDSM_ZONE_SIDE_BACKGROUND gives a background pixel that is in it other(p); one of side SDSM_ZONE_SIDE_OBJECT gives a
 * pixel of a label >= 1 that is in it L(p); with keep_own every pixel of a label >= 1 gets L(p); every other pixel gets 0.  So
 *   grown(hi)     = {BACKGROUND, 1, 0, hi}      ring(lo, hi) = {BACKGROUND, 0, lo, hi}
 *   core(lo)      = {OBJECT, 0, lo, SDSM_ZONE_NO_UPPER}      rim(hi) = {OBJECT, 0, 0, hi}
 * Every bound that is not SDSM_ZONE_NO_UPPER must be <= max_d2 (the search ends there); SDSM_ZONE_NO_UPPER is taken as hi_d2 of an
 * OBJECT zone only.
 * Conventions as for the tables above: sets as a HOST table of sdsm_set_image, int32 maps packed as the table says, the single-image
 * form is the set of that one image.  Every pixel of every map asked for is written, by plain stores of values that depend on the label
 * map alone: no output needs clearing.
 * Limits: labels 0 .. 65535 (a pixel with another label is counted in its image's status word and taken as label 0), H * H + W * W <
 * 2^31 per image, 1 .. SDSM_MAX_SET_IMAGES images, 0 .. SDSM_ZONE_MAX_ZONES zones. */
#define SDSM_ZONE_MAX_D2 4096
#define SDSM_ZONE_MAX_ZONES 8
#define SDSM_ZONE_NO_UPPER 0x7fffffff   /* hi_d2 of a zone without an upper bound */
#define SDSM_ZONE_SIDE_BACKGROUND 0
#define SDSM_ZONE_SIDE_OBJECT 1
typedef struct {
    int32_t side;                       /* SDSM_ZONE_SIDE_BACKGROUND or SDSM_ZONE_SIDE_OBJECT */
    int32_t keep_own;                   /* 1: every pixel of a label >= 1 keeps its label (BACKGROUND zones only); else 0 */
    int32_t lo_d2, hi_d2;               /* in the zone: lo_d2 < depth <= hi_d2; 0 <= lo_d2 < hi_d2 */
} sdsm_zone_spec;                       /* 16 bytes */
/* zones: a HOST array of n_zones specs.  d_d2, d_other: packed int32 maps as d_labels, either may be NULL (not written).  d_zone_out:
 * n_zones packed int32 maps, that of zone z from element z * zone_stride on; zone_stride >= offset + H * W of every image.  NULL with
 * n_zones == 0.  d_status: one int32 per image, cleared by the call: the pixels with a label outside 0 .. 65535. */
int sdsm_zones_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, int n_zones, const sdsm_zone_spec *zones,
                     int64_t zone_stride, int32_t *d_d2, int32_t *d_other, int32_t *d_zone_out, int32_t *d_status, void *stream);
int sdsm_zones(int H, int W, const int32_t *d_labels, int max_d2, int n_zones, const sdsm_zone_spec *zones, int32_t *d_d2, int32_t *d_other,
               int32_t *d_zone_out, int32_t *d_status, void *stream);   /* the set of one image; zone_stride = H * W */

/* ---- connected parts of one label map (no reference counterpart; the definitions are parts_host and keep_maps_host of
 * superdsm_amd/parts.py) ---------------------------------------------------------------------------------------------------------------
 * Which pixels of a label hang together, in integers only.  The map L (labels 0 .. 65535, 0 the background) is extended by label 0
 * outside the image frame.  A PART is a maximal set of pixels of one label >= 1 that are connected under the adjacency `connectivity`,
 * 4 or 8; pixels of different labels are never connected.  The parts of an image are numbered 1 .. K by their first pixel in raster
 * order (the smallest r * W + c), which for a map with the single label 1 is the numbering of scipy.ndimage.label.  The PART MAP holds
 * the part number of every pixel, 0 on the background.
 * Bit quads: q1, q3, qd of label l count, over all (H + 1) * (W + 1) windows of 2 x 2 places of the zero-padded mask L == l, those with
 * exactly one place of the mask, with exactly three, and with exactly the two places of a diagonal (sdsm_parts_quad).  The Euler number
 * of the mask is (q1 - q3 + 2 qd) / 4 under connectivity 4 and (q1 - q3 - 2 qd) / 4 under 8, and its holes are n_parts - Euler.
 * Conventions as for the zone maps: sets as a HOST table of sdsm_set_image, int32 maps packed as the table says, the single-image form
 * is the set of that one image.  Every pixel of every map is written by plain stores, every record by integer add / min / max atomics
 * on cleared records: the bytes do not depend on the order, the tiling, the launch or the set size.  No kernel waits for another
 * thread's progress.
 * Limits: labels 0 .. n_labels - 1, n_labels <= 65536 (a pixel with another label is counted in its image's status word and taken as
 * label 0), H * H + W * W < 2^31 per image, 1 .. SDSM_MAX_SET_IMAGES images, 0 .. SDSM_PARTS_MAX_KEEPS selections.  K is bounded by the
 * pixels alone; a part map goes into the other label-map entry points only while K <= 65535. */
#define SDSM_PARTS_MAX_KEEPS 8
#define SDSM_KEEP_SPLIT 0               /* a pixel of a label >= 1 gets its part number */
#define SDSM_KEEP_LARGEST 1             /* ... its label, if its part is largest_part of its label */
#define SDSM_KEEP_MIN_AREA 2            /* ... its label, if the area of its part is >= min_area */
typedef struct {
    int32_t label;                      /* the label of the part's pixels */
    int32_t area;
    int32_t first;                      /* raster index r * W + c of the part's first pixel */
    int32_t r0, c0, r1, c1;             /* the tight box, r1 and c1 exclusive */
    int32_t index_in_label;             /* NOT written by the device (0): the parts of a label counted in part order, by the caller */
} sdsm_part_record;                     /* 32 bytes */
typedef struct {
    int32_t n_parts;
    int32_t area;
    int32_t largest_area;
    int32_t largest_part;               /* the part number; of several parts of the largest area the smallest number */
    int32_t q1, q3, qd;                 /* bit-quad counts: at most (H + 1) * (W + 1) < 2^31 windows (H * W < 2^30, H + W < 2^17) */
    int32_t reserved;
} sdsm_part_label_record;               /* 32 bytes; the record of label 0 stays all zero */
typedef struct {
    int32_t kind;                       /* SDSM_KEEP_SPLIT, SDSM_KEEP_LARGEST or SDSM_KEEP_MIN_AREA */
    int32_t min_area;                   /* SDSM_KEEP_MIN_AREA: >= 1; else 0 */
} sdsm_keep_spec;                       /* 8 bytes */
/* Host helper (no device access), the inline function the tile kernel uses (csrc/sdsm_parts.h): the class of the window  a b / c d
 * against the mask of `label`: 0 none, 1 q1, 2 q3, 3 qd. */
int sdsm_parts_quad(int32_t a, int32_t b, int32_t c, int32_t d, int32_t label);
/* LABELLING.  d_label_out[rec_off[i] + l] for the labels 0 <= l < n_labels[i] of image i (rec_off, n_labels: HOST arrays, as
 * sdsm_neighbours_multi takes them), complete; d_part_map: the packed int32 part maps; d_count: one int32 per image, its K; d_status:
 * one int32 per image, the pixels with a label < 0 or >= n_labels.  The call clears what it adds into, on the stream.  d_ws: at least
 * sdsm_parts_workspace_bytes_multi bytes, 8-byte aligned (parents, part areas, scan chunks, the keys of the largest parts).
 * K is not known before the scan, so the part table is a call of its own, once the caller has read d_count. */
size_t sdsm_parts_workspace_bytes_multi(const sdsm_set_image *images, int n_images, const int64_t *rec_off, const int32_t *n_labels);
int sdsm_parts_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int connectivity, const int64_t *rec_off,
                     const int32_t *n_labels, sdsm_part_label_record *d_label_out, int32_t *d_part_map, int32_t *d_count, int32_t *d_status,
                     void *d_ws, size_t ws_bytes, void *stream);
int sdsm_parts(int H, int W, const int32_t *d_labels, int connectivity, int n_labels, sdsm_part_label_record *d_label_out, int32_t *d_part_map,
               int32_t *d_count, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream);   /* the set of one image */
/* PART TABLE.  d_part_out[part_off[i] + k - 1] for the parts 1 <= k <= n_parts[i] of image i (part_off, n_parts: HOST arrays; n_parts as
 * read from d_count; the ranges must not overlap), from the label map and the part map of sdsm_parts_multi.  A pixel whose part number
 * lies outside 1 .. n_parts is passed over.  The call initialises the records on the stream. */
int sdsm_parts_table_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map, const int64_t *part_off,
                           const int32_t *n_parts, sdsm_part_record *d_part_out, void *stream);
/* SELECTIONS.  keeps: a HOST array of n_keeps specs.  d_keep_out: n_keeps packed int32 maps, that of selection z from element
 * z * keep_stride on; keep_stride >= offset + H * W of every image.  Reads the two maps and the two tables of the calls above; every pixel
 * of every map is written.  A pixel whose label lies outside 1 .. n_labels - 1 or whose part lies outside 1 .. n_parts gets 0. */
int sdsm_parts_keep_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map, const int64_t *rec_off,
                          const int32_t *n_labels, const sdsm_part_label_record *d_label_recs, const int64_t *part_off, const int32_t *n_parts,
                          const sdsm_part_record *d_part_recs, int n_keeps, const sdsm_keep_spec *keeps, int64_t keep_stride, int32_t *d_keep_out,
                          void *stream);

/* ---- depth tables: inscribed circle, radii, intensity shells (no reference counterpart; the definitions are depth_objects_host and
 * depth_labels_host of superdsm_amd/depth.py) ---------------------------------------------------------------------------------------------
 * How far inside its object a pixel lies, in integers only.  An object is the set P of the set bits of its fragment, as in the shape
 * tables; everything else -- the rest of its box, other objects or labels, the outside of the image -- is outside P.  d2(p) for p in P
 * is the smallest squared Euclidean distance from p to a lattice place outside P; a place one step beyond the image frame, or beyond the
 * box, counts like any other outside pixel.  So d2 >= 1 for every p in P, and d2 <= ceil(min(h, w) / 2)^2 over the tight box.
 * Conventions as for the shape and intensity tables: objects as sdsm_post_objects takes them, sets as a HOST table of sdsm_set_image
 * (H, W <= 65535, H * W < 2^31), the single-image form is the set of that one image.  Every sum is an integer sum and every LDS atomic an
 * integer add, there is no global atomic, and every record and shell row is written completely by its own workgroup: the bytes do not
 * depend on the order, the launch or the set size, and no output needs clearing.
 *
 * Ranges: min(h, w) <= 65535 gives d2 <= 32768^2 = 2^30, and area <= h * w < 2^31, so sum_d2 <= area * max_d2 < 2^61; q(d2) =
 * floor(sqrt(d2 * 2^32)) <= 2^31 (sdsm_quantised_distance, the one function the boundary tables use), so sum_q < 2^62.  Neither sum can
 * wrap an int64, and neither is split into limbs.
 * Median: med_d2_lo, med_d2_hi are the order statistics of d2 at the two ranks of the quantile 1 / 2 (sdsm_quantile_ranks(area, 1, 2)).
 * Shells: with 1 <= n_shells <= SDSM_DEPTH_MAX_SHELLS the shell of a pixel is min(n_shells - 1, isqrt(d2 - 1)), that is ceil(sqrt(d2)) - 1
 * capped: shell 0 holds d2 == 1, shell 1 d2 in 2 .. 4, shell 2 d2 in 5 .. 9, the last shell every deeper pixel (sdsm_depth_shell).
 * Intensities (d_g, float64, optional) enter as for the measurement tables: e is the image's scale exponent, found on the device by the
 * same first kernel (d_gmax_abs, d_scale_exp as sdsm_measure_objects takes them), a finite pixel adds q = rint(ldexp(g, 62 - e)) in two
 * limbs to its shell, a non-finite pixel is counted in `count` alone.  Without d_g only `count` is filled and scale_exp is 0.
 * An object whose box holds at most SDSM_DEPTH_LDS_PIXELS pixels is transformed in LDS; a larger one needs
 * sdsm_depth_workspace_pixels(h, w) pixels of SDSM_DEPTH_WS_PIXEL_BYTES bytes each in the caller's workspace: the same bytes, more slowly
 * (see DESIGN.md "Limits").  The decision is by the box, not by the pixels in it.  sdsm_depth_record: 80 bytes; sdsm_depth_shell_record:
 * 32 bytes. */
#define SDSM_DEPTH_MAX_SHELLS 32
#define SDSM_DEPTH_LDS_PIXELS 12288     /* pixels of a box whose transform is held in LDS (two uint16 tiles, 48 KB) */
#define SDSM_DEPTH_WS_PIXEL_BYTES 8     /* bytes of workspace per pixel of a larger box (two uint32) */
#define SDSM_DEPTH_NO_WORKSPACE (1 << 30)   /* flag bit 30 of sdsm_depth_record */
typedef struct {
    int64_t area;                       /* pixels of P */
    int64_t max_d2;                     /* largest d2: the squared radius of the largest inscribed circle */
    int32_t max_row, max_col;           /* the pixel with d2 == max_d2 that is smallest in (row, column) order, image coordinates */
    int64_t n_max;                      /* pixels with d2 == max_d2 */
    int64_t sum_d2;                     /* sum of d2, < 2^61 */
    int64_t sum_q;                      /* sum of q(d2), < 2^62 */
    int64_t med_d2_lo, med_d2_hi;       /* the two middle order statistics of d2 */
    int64_t n_rim;                      /* pixels with d2 == 1: the border pixels of the shape tables */
    int32_t flags;                      /* bit 0: the bounding box of P touches the image frame; bit 30: the box needs workspace and the
                                           call names none for it (the record and its shells are then zero) */
    int32_t scale_exp;                  /* e of the record's image; 0 without d_g and in the zero record */
} sdsm_depth_record;
typedef struct {
    int64_t count;                      /* pixels of the shell */
    int64_t n_finite;                   /* those with a finite intensity */
    uint64_t gsum_lo;                   /* low limb of their intensity sum */
    int64_t gsum_hi;                    /* high limb */
} sdsm_depth_shell_record;
/* Host helpers (no device access).  sdsm_depth_shell: the shell of d2 among n_shells, by the inline function the kernel uses
 * (csrc/sdsm_depth.h: a float estimate of the root, then integer correction loops); -1 for d2 < 1, d2 >= 2^31 or n_shells outside
 * 1 .. SDSM_DEPTH_MAX_SHELLS.  sdsm_depth_workspace_pixels: the workspace pixels an object with an h x w box needs, h * w above
 * SDSM_DEPTH_LDS_PIXELS and 0 for a box that LDS holds or an empty one. */
int sdsm_depth_shell(int64_t d2, int n_shells);
int64_t sdsm_depth_workspace_pixels(int h, int w);
/* d_out[i] and d_shells[i * n_shells + s] for object i of d_boxes / d_bits_off (n of them; d_obj_image int32, NULL for one image), one
 * workgroup each.  The bits of a fragment past h * w are ignored, a box larger than the tight box changes nothing; a fragment without a
 * set bit, and an object whose box is empty or leaves its image, give the zero record and zero shells, and nothing is read for them.
 * Workspace: object i with sdsm_depth_workspace_pixels(h, w) > 0 owns that many pixels of d_ws from pixel d_ws_off[i] on (d_ws_off: n
 * int64 on the device; entries of smaller objects are not read; the ranges must not overlap, which is the caller's duty: the offsets
 * live on the device and an overlap is not detected); ws_pixels is the number of pixels the offsets name in all and ws_bytes the size
 * of d_ws: ws_pixels * SDSM_DEPTH_WS_PIXEL_BYTES > ws_bytes is an argument error before any
 * launch, and an object whose range does not lie in 0 .. ws_pixels gets flag bit 30.  d_ws_off and d_ws may be NULL with ws_pixels ==
 * 0.  d_g NULL: d_gmax_abs and d_scale_exp may be NULL.  n == 0: no launch. */
int sdsm_depth_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                       double *d_gmax_abs, int32_t *d_scale_exp, int n_shells, const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels,
                       size_t ws_bytes, sdsm_depth_record *d_out, sdsm_depth_shell_record *d_shells, void *stream);
int sdsm_depth_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                             const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                             int n_shells, const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, size_t ws_bytes, sdsm_depth_record *d_out,
                             sdsm_depth_shell_record *d_shells, void *stream);
/* The same for labels of label maps, by the windows of sdsm_shape_labels: the caller names n windows (d_obj_image, d_boxes, d_bits_off
 * into the workspace d_bits of window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS words, which the call clears) and d_label_obj; a first kernel
 * sets the bit of every pixel in the window of its label -- a pixel of another label stays outside --, then the windows are measured as
 * objects.  d_bad as there. */
int sdsm_depth_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                      const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, double *d_gmax_abs,
                      int32_t *d_scale_exp, int n_shells, const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, size_t ws_bytes,
                      sdsm_depth_record *d_out, sdsm_depth_shell_record *d_shells, int32_t *d_bad, void *stream);
int sdsm_depth_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                            const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                            int64_t window_words, uint32_t *d_bits, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp, int n_shells,
                            const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, size_t ws_bytes, sdsm_depth_record *d_out,
                            sdsm_depth_shell_record *d_shells, int32_t *d_bad, void *stream);

/* ---- skeleton tables: midlines, end and branch points, length (no reference counterpart; the definitions are skeleton_objects_host and
 * skeleton_labels_host of superdsm_amd/skeleton.py) ----------------------------------------------------------------------------------------
 * The form of an object along its own midline, in integers only.  An object is the set P of the set bits of its fragment; everything
 * else -- the rest of its box, other objects or labels, the outside of the image -- is 0.
 * Neighbourhood code: bit k of code(p) is the pixel at offset k of the ring, clockwise from north: N(-1,0), NE(-1,1), E(0,1), SE(1,1),
 * S(1,0), SW(1,-1), W(0,-1), NW(-1,-1); x_k is that bit, indices modulo 8.
 * Removal rule: for a direction d of N, S, E, W (ring bits 0, 4, 2, 6) deletable(code, d) holds iff x_d = 0 (a border pixel on side d),
 * the 8-connectivity number sum over k in {0, 2, 4, 6} of (1 - x_k) (x_{k+1} | x_{k+2}) is 1 (the pixel is simple), and at least two of
 * the eight x_k are set (neither an end nor isolated).  41 of the 256 codes are deletable per direction.
 * Thinning: a subiteration for d removes, simultaneously, every pixel of X with deletable(code, d), the codes taken before any removal
 * of that subiteration; a cycle is the four subiterations N, S, E, W; the skeleton S of P is X after repeating cycles from X = P until
 * one whole cycle removes nothing, and `cycles` counts the cycles that removed a pixel.  S is a subset of P with the 8-connected parts
 * and the holes of P.
 * The kernel thins a box of at most 64 x 64 in the registers of one wavefront, a box of at most SDSM_SKELETON_LDS_WORDS row-aligned
 * 64-bit words (h * ceil(w / 64)) in LDS, and a larger one in sdsm_skeleton_workspace_words(h, w) 64-bit words of the caller's workspace:
 * the same bytes, more slowly (see DESIGN.md "Limits").  The decision is by the box, not by the pixels in it.  Every count is an
 * integer, there is no atomic, and every record and skeleton window is written completely by its own wavefront or workgroup: the bytes
 * do not depend on the order, the launch or the set size.  sdsm_skeleton_record: 48 bytes. */
#define SDSM_SKELETON_LDS_WORDS 3072    /* 64-bit words of a box whose thinning is held in LDS (two planes, 48 KB: three workgroups a CU) */
#define SDSM_SKELETON_NO_WORKSPACE (1 << 30)   /* flag bit 30 of sdsm_skeleton_record */
typedef struct {
    int32_t area;                       /* pixels of P */
    int32_t n_skeleton;                 /* pixels of S */
    int32_t n_end;                      /* pixels of S with exactly one ring neighbour in S */
    int32_t n_isolated;                 /* pixels of S with none */
    int32_t n_branch;                   /* pixels of S with >= 3 transitions 0 -> 1 around their ring in S */
    int32_t n_orth;                     /* unordered pairs of 4-adjacent pixels of S */
    int32_t n_diag;                     /* unordered pairs of diagonally adjacent pixels of S whose two common 4-neighbours are outside S */
    int32_t cycles;                     /* cycles that removed a pixel */
    int32_t first_row, first_col;       /* the first pixel of S in raster order, image coordinates */
    int32_t flags;                      /* bit 0: the bounding box of P touches the image frame; bit 30: the box needs workspace and the call
                                           names none for it (the record is then zero and its skeleton window is not written) */
    int32_t reserved;                   /* 0 */
} sdsm_skeleton_record;
/* Host helpers (no device access), by the inline functions the kernel uses (csrc/sdsm_skeleton.h).  sdsm_skeleton_deletable: the removal
 * rule, 1 or 0; -1 for a code outside 0 .. 255 or a direction that is none of 0, 2, 4, 6.  sdsm_skeleton_workspace_words: the 64-bit
 * workspace words an object with an h x w box needs, 2 h ceil(w / 64) above SDSM_SKELETON_LDS_WORDS and 0 for a box that LDS or a
 * wavefront holds or an empty one.  sdsm_skeleton_thin: thins one flat-packed h x w window (bit r w + c of ceil(h w / 32) uint32 words;
 * the bits past h w are ignored) on the CPU with the header's word functions into `skeleton` (the same layout, the bits past h w clear;
 * it may be `bits` itself); returns `cycles`, or -1 for h < 1, w < 1, h w >= 2^31 or a null argument. */
int sdsm_skeleton_deletable(int code, int direction);
int64_t sdsm_skeleton_workspace_words(int h, int w);
int sdsm_skeleton_thin(int h, int w, const uint32_t *bits, uint32_t *skeleton);
/* d_out[i] and the skeleton window of object i of d_boxes / d_bits_off (n of them; d_obj_image int32, NULL for one image).  d_skeleton:
 * as many words as d_bits, the window of object i at d_bits_off[i] in the layout of its fragment; its contents do not matter.  The bits of a
 * fragment past h * w are ignored; a fragment without a set bit gives the zero record and a clear window; an object whose box is empty or
 * leaves its image gives the zero record, and nothing is read or written for it.  Workspace: object i with
 * sdsm_skeleton_workspace_words(h, w) > 0 owns that many 64-bit words of d_ws from word d_ws_off[i] on (d_ws_off: n int64 on the device;
 * entries of smaller objects are not read; the ranges must not overlap, which is the caller's duty); ws_words is the number of words the
 * offsets name in all and ws_bytes the size of d_ws: ws_words * 8 > ws_bytes is an argument error before any launch, and an object whose
 * range does not lie in 0 .. ws_words gets flag bit 30.  d_ws_off and d_ws may be NULL with ws_words == 0.  n == 0: no launch. */
int sdsm_skeleton_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_ws_off,
                          void *d_ws, int64_t ws_words, size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, void *stream);
int sdsm_skeleton_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_ws_off, void *d_ws, int64_t ws_words,
                                size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, void *stream);
/* The same for labels of label maps, by the windows of sdsm_shape_labels: the caller names n windows (d_obj_image, d_boxes, d_bits_off
 * into the workspace d_bits of window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS words, which the call clears) and d_label_obj; a first kernel
 * sets the bit of every pixel in the window of its label -- a pixel of another label is outside --, then the windows are thinned as
 * objects.  d_obj_label: the label of window i (n int32).  d_map (int32, the layout of d_labels; may be NULL) is cleared in stream order,
 * then every skeleton pixel receives its label.  d_bad as there. */
int sdsm_skeleton_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                         const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const int32_t *d_obj_label, const int64_t *d_ws_off,
                         void *d_ws, int64_t ws_words, size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, int32_t *d_map,
                         int32_t *d_bad, void *stream);
int sdsm_skeleton_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                               const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                               int64_t window_words, uint32_t *d_bits, const int32_t *d_obj_label, const int64_t *d_ws_off, void *d_ws,
                               int64_t ws_words, size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, int32_t *d_map, int32_t *d_bad,
                               void *stream);

/* ---- host-side combinatorial steps of the stage (no device access) -------------------------------------------------------------
 * Approximate min-weight set cover (superdsm/minsetcover.py:4-88: greedy + merge phase, retried with beta * gamma on up to max_iter
 * levels) and greedy max-weight set packing (superdsm/maxsetpack.py:8-24) over n objects whose footprints are bit sets of `words`
 * uint64 each (bit = atom of the cluster); same decisions, arithmetic and tie-breaking as the reference's Python.  selected
 * receives the indices of the solution in the reference's list order, n_selected their number. */
int sdsm_minsetcover(int n, int words, const uint64_t *footprints, const double *energies, double beta, int merge, int max_iter,
                     double gamma, int32_t *selected, int32_t *n_selected);
int sdsm_maxsetpack(int n, int words, const uint64_t *footprints, const double *energies, int32_t *selected, int32_t *n_selected);
/* sdsm_minsetcover for several independent families in one call (MinSetCover.update, superdsm/minsetcover.py:142-153: one cover per touched
 * cluster): family f has n[f] objects of words[f] uint64; footprints / energies / selected of the families follow each other (n[f] *
 * words[f] / n[f] / n[f] entries); n_selected[f] = size of family f's solution. */
int sdsm_minsetcover_multi(int n_families, const int32_t *n, const int32_t *words, const uint64_t *footprints, const double *energies, double beta,
                           int merge, int max_iter, double gamma, int32_t *selected, int32_t *n_selected);

/* Host helper (no device access): size of the search space of the stage's iterations, per cluster -- what the reference's
 * _estimate_progress (superdsm/globalenergymin.py:310-323) enumerates footprint by footprint in Python from the generation of the
 * atoms on: the number of footprints that growing by one adjacent atom at a time produces (_iterate_generation,
 * globalenergymin.py:292-307; skip_last: the universe of a cluster is not counted).  Atoms of cluster k: offsets[k] .. offsets[k+1]-1;
 * adj / compat: per atom, the bit set (local indices within its cluster) of its adjacent atoms / of the atoms within
 * max_seed_distance of it (NULL: no limit).  counts[k] = -1 for clusters of more than 64 atoms.  Counting stops once the total
 * exceeds max_amount. */
int sdsm_count_growth(int n_clusters, const int32_t *offsets, const uint64_t *adj, const uint64_t *compat, int skip_last,
                      int64_t max_amount, int64_t *counts);

/* Host helper (no device access): the foreground fragments (objects.py:148-174) of a batch out of the downloaded records and
 * bit-packed masks, one byte per pixel: fragment i (fg_h x fg_w, row-major) at out + out_offset[i]; candidates without a
 * foreground get the single byte 0 ([[False]], objects.py:172-174).  Returns the bytes written -- or needed, when out == NULL. */
int64_t sdsm_unpack_fragments(const sdsm_record *records, const int32_t *mask_info, const int64_t *mask_offset, const uint8_t *masks,
                              int n, uint8_t *out, int64_t *out_offset);

/* Parity / debug: psi, its gradient and the polynomial (theta) block of its Hessian at caller-given parameters, computed
 * by the evaluators of the solve kernels (Energy.__call__ / grad / hessian, superdsm/dsm.py:312-385) on the crops and G~
 * rows that a previous sdsm_batch_launch of the same plan left in the workspace.  d_params: sdsm_plan_eval_param_count()
 * doubles, candidate i's vector (theta[6] in full-image-normalised coordinates, then xi[M]) at 6 * i + xi_offset[i].
 * d_out: sdsm_plan_eval_out_count() doubles: [2 i], [2 i + 1] psi by the full and by the value-only evaluator;
 * [2 n + 21 i ..] lower triangle (row-major) of the 6x6 theta block of the Hessian; [23 n + 6 i + xi_offset[i] ..] the
 * gradient in the layout of d_params.  Candidates without a solve (trivial, failed, beyond the limits) get NaN. */
/* Callable dsm/init (reference: superdsm/objects.py:385-386, `params = init(J.smooth_mat.shape[1])`): the caller's own starting point of
 * the DSM solve instead of the elliptical model's optimum.  The number of columns of a candidate's G~ -- its grid points -- is a result
 * of the setup kernel: sdsm_batch_deform_counts runs it alone (arguments as sdsm_batch_launch_multi), SYNCHRONISES the stream and writes
 * n_deform[i] = M of candidate i to host memory (-1: no solve -- trivial region, failed setup; 0 also for a system beyond the solver's
 * limit, which gets the elliptical model only).  sdsm_plan_set_start then names the starting points of the following launches: d_x0 =
 * sdsm_plan_eval_param_count() doubles on the device, candidate i's theta[6] (full-image-normalised) + xi[M] at 6 * i + xi_offset[i]
 * (the layout of sdsm_batch_eval's d_params); it must stay valid until those launches have completed; NULL = none.  Only for plans with
 * init_elliptical = 0 (SDSM_ERR_ARGUMENT otherwise); a candidate whose solve falls back (SDSM_CAND_FALLBACK) returns the initialisation. */
int sdsm_batch_deform_counts(const sdsm_plan *plan, const double *const *d_y, const int32_t *const *d_atoms, const uint8_t *const *d_valid,
                             void *d_workspace, size_t workspace_bytes, int32_t *n_deform, void *stream);
int sdsm_plan_set_start(const sdsm_plan *plan, const double *d_x0);
int64_t sdsm_plan_eval_param_count(const sdsm_plan *plan);
int64_t sdsm_plan_eval_out_count(const sdsm_plan *plan);
int sdsm_batch_eval(const sdsm_plan *plan, void *d_workspace, size_t workspace_bytes, const double *d_params, double *d_out, void *stream);
/* Parity / debug: ONE damped Newton step as the solver takes it, piece by piece, at caller-given parameters (no reference counterpart:
 * the reference hands its energy to cvxopt; DESIGN.md "Solver").  Like sdsm_batch_eval it works on the workspace of a previous
 * sdsm_batch_launch of the same plan and takes d_params in that call's layout; d_dir (same layout, NULL = none) is a search direction.
 * The solver's own functions run in the LDS layout, thread count and Hessian placement of ONE solve class, `layout`:
 *   SDSM_STEP_LAYOUT_1 class 1, throughput mode (192 threads)   _1_LATENCY class 1, 256 threads   _1B   _2   _2B
 *   _3 (Hessian in global memory: only candidates the plan reserved a slot for)   _LIGHT a light group member's layout, alone.
 * Everything is returned in the candidate's LOCAL frame (coordinates centred on its box and scaled by its half extents -- the frame the
 * solve kernels work in; theta_local is linear in theta), unknowns in the order theta[6], xi[M], and nothing is computed on top of what
 * the solver's functions return.  Candidate i's block starts at d_out + i * stride doubles (SDSM_STEP_*), n = 6 + M:
 *   [SDSM_STEP_RC]        return code of the factorisation (0 ok, 1 not positive definite, 2 non-finite); -1: the candidate has no solve,
 *                         does not fit the layout, or its block does not fit `stride` -- the rest of its block is then NaN
 *   [SDSM_STEP_PSI_VALUE] psi by the value-only evaluator   [SDSM_STEP_PSI] psi by the full evaluation (regulariser curvature blended by
 *                         reg_mu in [0, 1], sums scaled by the bound psi_value)   [SDSM_STEP_LAM2] -g.d of the step (NaN unless RC = 0)
 *   [SDSM_STEP_N] n   [SDSM_STEP_ENV] E, the doubles of the Hessian envelope (21 for M = 0: the packed lower triangle of the 6 x 6 matrix)
 *   [SDSM_STEP_LINE .. + 3] psi(x + t d) for t = t0, t0 / 2, t0 / 4, t0 / 8 by the line-search sweep, along d_dir if given, else along
 *                         the Newton direction (NaN if there is neither)
 *   [SDSM_STEP_HEAD ..]   gradient[n]; Newton direction[n], the solution of (H + tau diag H) d = -g (NaN unless RC = 0); envelope[E] as the
 *                         full evaluation left it, BEFORE the factorisation; then, as int32: rb[n], fst[n], rend[ceil(M / 4)] -- unknowns in
 *                         the envelope's order (xi[M], then theta[6]), row a holds columns fst[a] .. a at envelope[rb[a] + column];
 *                         rend[p]: the last xi row that reaches the columns of panel p.
 * A block needs SDSM_STEP_HEAD + 2 n + E + (2 n + ceil(M / 4) + 1) / 2 doubles.  d_out (n_candidates * stride doubles) is filled with
 * NaN first.  Asynchronous on `stream`. */
enum { SDSM_STEP_LAYOUT_1 = 0, SDSM_STEP_LAYOUT_1_LATENCY, SDSM_STEP_LAYOUT_1B, SDSM_STEP_LAYOUT_2, SDSM_STEP_LAYOUT_2B, SDSM_STEP_LAYOUT_3, SDSM_STEP_LAYOUT_LIGHT, SDSM_STEP_LAYOUT_N };
enum { SDSM_STEP_RC = 0, SDSM_STEP_PSI_VALUE = 1, SDSM_STEP_PSI = 2, SDSM_STEP_LAM2 = 3, SDSM_STEP_N = 4, SDSM_STEP_ENV = 5, SDSM_STEP_LINE = 6, SDSM_STEP_HEAD = 10 };
int sdsm_batch_eval_step(const sdsm_plan *plan, void *d_workspace, size_t workspace_bytes, int layout, double reg_mu, double tau, double t0,
                         const double *d_params, const double *d_dir, double *d_out, int64_t stride, void *stream);
/* Parity / debug: the scalar arithmetic every pass over the pixels goes through, element by element -- the device functions of the
 * solve kernels as compiled (no host copy), with the table of the logarithm where those kernels keep it.  d_y, d_S, d_x: n doubles each
 * (device memory), 0 <= n <= SDSM_PROBE_LOSS_MAX; d_out: SDSM_PROBE_N arrays of n doubles, array k at d_out + k * n.  With
 * t = d_y[i] * d_S[i] and u = exp_neg(min(|t|, 750)) (a NaN t counts as 750, as in the kernels):
 *   SDSM_PROBE_T t   SDSM_PROBE_EXP u   SDSM_PROBE_LOG log_w(u, 1 + u)   SDSM_PROBE_SOFTPLUS softplus_neg(t) = log(1 + exp(-t))
 *   SDSM_PROBE_PHI / _R / _DCURV the three results of loss_terms(d_y[i], d_S[i]): phi = log(1 + exp(-t)), r = -y theta with
 *   theta = 1 / (1 + exp(t)), dcurv = y^2 u / (1 + u)^2   SDSM_PROBE_RCP rcp_f64(d_x[i])   SDSM_PROBE_RSQRT rsqrt_f64(d_x[i])
 * Asynchronous on `stream`. */
#define SDSM_PROBE_LOSS_MAX (1 << 20)
enum { SDSM_PROBE_T = 0, SDSM_PROBE_EXP, SDSM_PROBE_LOG, SDSM_PROBE_SOFTPLUS, SDSM_PROBE_PHI, SDSM_PROBE_R, SDSM_PROBE_DCURV, SDSM_PROBE_RCP, SDSM_PROBE_RSQRT, SDSM_PROBE_N };
int sdsm_probe_loss_arithmetic(int64_t n, const double *d_y, const double *d_S, const double *d_x, double *d_out, void *stream);

/* Timing of the dominant kernel with HIP events on the launch stream: after sdsm_batch_launch returns,
 * sdsm_last_solve_kernel_ms() synchronises on the recorded events and returns the solve kernels' duration. */
int sdsm_enable_kernel_timing(int enable);
double sdsm_last_solve_kernel_ms(void);
double sdsm_last_setup_kernel_ms(void);
/* Solver diagnostics of the production build, process-wide, taken by every following launch: bit 0 = a second full evaluation at an
 * unchanged iterate repeats the pass over the pixels instead of taking the sums the first one kept.  Results do not depend on it (the
 * tests compare).  An unknown bit: SDSM_ERR_ARGUMENT.  sdsm_batch_solver_counters synchronises the device and reads the event
 * counters of the plan's last launch on this workspace (0 before any): out[0] full evaluations served from kept sums, out[1 .. 3] 0. */
int sdsm_set_solver_diagnostics(int flags);
int sdsm_batch_solver_counters(const sdsm_plan *plan, void *d_workspace, int64_t out[4]);
/* Diagnostic builds only (-DSDSM_PROFILE): device buffer receiving 8 int64 cycle counters per candidate
 * (phase A, phase B, reductions, factor+solve, line search, total, elliptical total, reserved). */
int sdsm_set_debug_buffer(void *d_buf);
/* Microseconds a member of a workgroup group waits for its partners at one exchange before the group gives its candidate up
 * (SDSM_CAND_GIVEN_UP: the caller solves it again in a plan without groups, sdsm_plan_set_latency_mode(plan, 2)); <= 0 restores the
 * default of 50 ms.  Applies to the launches of the calling thread. */
int sdsm_set_group_timeout_us(double us);
/* A launch runs its solve classes on the caller's stream and three side streams of the library (four for plans whose class 2b has a queue
 * of its own), which must sit on different hardware queues (HIP's default of 4 suffices).  The library keeps a pool of up to 8 side
 * streams per device and, the first time it sees a caller stream, probes which of them run side by side with that stream and with each
 * other (before any work of that launch is queued; it synchronises the caller's stream once).  Of the last launch of this process that
 * needed side streams -- 1: they run side by side; 0: fewer than three side streams with a queue of their own were found -- launches are
 * correct but classes run one after the other, a warning went to stderr once; -1: not known (no such launch yet, or the probe stayed
 * undecided on a busy chip: it is repeated at later launches).  No reference counterpart (the reference's parallelism is Ray,
 * objects.py:270-284). */
int sdsm_side_queues_distinct(void);
/* The same launch in figures: out[0] streams in the pool, out[1] side streams with a queue of their own found for the caller's stream,
 * out[2] probes made so far, out[3 .. 6] pool indices used for side 1 .. 4 (-1: none), out[7] probes that stayed undecided so far. */
int sdsm_side_queue_report(int32_t out[8]);
/* The choice itself as a pure host function (no GPU): shares is an (n_pool + 1) x (n_pool + 1) "share a hardware queue" relation, index 0
 * the caller's stream, 1 + i pool stream i, read symmetrically.  Greedy in pool order: a stream is taken if it shares with neither the
 * caller's stream nor a stream taken before, until `want` are found; returns how many were found and writes `want` pool indices to out.
 * Missing ones are replaced: out[2] = out[1] (class 1b behind the groups / class 2), then out[1] = out[0]; nothing found: pool stream 0
 * throughout; entries from the fourth on, and every entry of an empty pool: -1.  Returns -1 for a bad argument. */
int sdsm_choose_sides_host(int n_pool, const uint8_t *shares, int want, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* SDSM_H */
