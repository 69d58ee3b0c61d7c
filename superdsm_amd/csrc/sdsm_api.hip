// Host side of the C ABI (include/sdsm.h): the entry points that touch the device -- upload, launch, point evaluation, probes, timing -- and the
// argument-checking wrappers of the other kernel files.  The plan and its workspace: sdsm_plan.hip; the side streams: sdsm_sides.hip.  No device
// allocation happens here: every device buffer is provided by the caller.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sdsm_sides.h"

extern "C" hipError_t sdsm_image_prepare_impl(const double *, const uint8_t *, const int32_t *, int, int, double, int, uint8_t *, int32_t *, void *, hipStream_t);
extern "C" hipError_t sdsm_preprocess_impl(const double *, int, int, double, double, double, int, double *, void *, hipStream_t);
static int hipfail(hipError_t e, const char *what) { return fail(SDSM_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" int sdsm_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { hipfail(e, "hipGetDeviceCount"); return 0; }
    return n;
}

extern "C" int sdsm_set_device(int device)
{
    hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "hipSetDevice");
}

extern "C" int sdsm_stream_synchronize(void *stream)
{
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "hipStreamSynchronize");
}

// ---- preprocessing / image prepare --------------------------------------------------------------------
extern "C" size_t sdsm_preprocess_workspace_bytes(int H, int W, double sigma1, double sigma2);
extern "C" size_t sdsm_image_workspace_bytes(int H, int W);

extern "C" int sdsm_preprocess(const double *d_g, int H, int W, double sigma1, double sigma2, double offset_clip, int lower_clip_mean,
                               double *d_y, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!d_g || !d_y || H < 1 || W < 1 || !(sigma1 > 0) || !(sigma2 > 0)) return fail(SDSM_ERR_ARGUMENT, "sdsm_preprocess: bad argument");
    if (ws_bytes < sdsm_preprocess_workspace_bytes(H, W, sigma1, sigma2) || !d_ws) return fail(SDSM_ERR_WORKSPACE, "sdsm_preprocess: workspace too small");
    hipError_t e = sdsm_preprocess_impl(d_g, H, W, sigma1, sigma2, offset_clip, lower_clip_mean, d_y, d_ws, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_preprocess");
}

extern "C" int sdsm_image_prepare(const double *d_y, const uint8_t *d_y_mask, const int32_t *d_atoms, int H, int W, double margin,
                                  int n_atoms, uint8_t *d_valid, int32_t *d_atom_stats, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!d_y || !d_atoms || !d_valid || !d_atom_stats || H < 2 || W < 2 || H > 65535 || W > 65535 || n_atoms < 0)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_image_prepare: bad argument (image must be 2..65535 pixels per side)");
    if (n_atoms > SDSM_MAX_LABELS) return fail(SDSM_ERR_UNSUPPORTED, "sdsm_image_prepare: more than 65535 atom labels");
    if (!(margin >= 0)) return fail(SDSM_ERR_ARGUMENT, "sdsm_image_prepare: background_margin must be >= 0");
    if (ws_bytes < sdsm_image_workspace_bytes(H, W) || !d_ws) return fail(SDSM_ERR_WORKSPACE, "sdsm_image_prepare: workspace too small");
    hipError_t e = sdsm_image_prepare_impl(d_y, d_y_mask, d_atoms, H, W, margin, n_atoms, d_valid, d_atom_stats, d_ws, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_image_prepare");
}

extern "C" int sdsm_batch_upload(const sdsm_plan *p, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!p || !d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_upload: null argument");
    if (ws_bytes < p->total) return fail(SDSM_ERR_WORKSPACE, "sdsm_batch_upload: workspace too small");
    if (p->n == 0) { p->uploaded_gen = p->layout_gen; p->uploaded_ws = d_ws; return SDSM_OK; }
    const BatchParams P = make_params(p, d_ws);          // the typed pointers of the blocks
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemcpyAsync((void *)P.cand, p->cand.data(), sizeof(CandDesc) * p->n, hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload cand");
    if (!p->fp_labels.empty() && (e = hipMemcpyAsync((void *)P.fp_labels, p->fp_labels.data(), sizeof(*P.fp_labels) * p->fp_labels.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload footprints");
    if ((e = hipMemcpyAsync((void *)P.order, p->order.data(), sizeof(*P.order) * p->order.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload order");
    if ((e = hipMemcpyAsync((void *)P.psf, p->psf.data(), sizeof(*P.psf) * p->psf.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload psf");
    if ((e = hipMemsetAsync(ws_words(p, d_ws), 0, sizeof(LaunchWords), s)) != hipSuccess) return hipfail(e, "hipMemsetAsync");   // (the event counters read 0 before the first launch)
    p->uploaded_gen = p->layout_gen; p->uploaded_ws = d_ws;
    return SDSM_OK;
}

extern "C" int sdsm_solve_wants_own_2b(int n_w, int n_d);

static thread_local int g_timing = 0;
static thread_local hipEvent_t g_ev[3] = {nullptr, nullptr, nullptr};
static thread_local int g_ev_valid = 0;

extern "C" int sdsm_enable_kernel_timing(int enable)
{
    g_timing = enable;
    if (enable && !g_ev[0]) {
        for (int i = 0; i < 3; i++) { hipError_t e = hipEventCreate(&g_ev[i]); if (e != hipSuccess) return hipfail(e, "hipEventCreate"); }
    }
    return SDSM_OK;
}

static double elapsed(int a, int b)
{
    if (!g_ev_valid) return -1.0;
    if (hipEventSynchronize(g_ev[b]) != hipSuccess) return -1.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, g_ev[a], g_ev[b]) != hipSuccess) return -1.0;
    return ms;
}
extern "C" double sdsm_last_setup_kernel_ms(void) { return elapsed(0, 1); }

extern "C" int sdsm_batch_solver_counters(const sdsm_plan *p, void *d_ws, int64_t out[4])
{
    if (!p || !d_ws || !out) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_solver_counters: null argument");
    if (p->uploaded_ws != d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_solver_counters: not the workspace of the plan's upload (sdsm_batch_upload)");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (p->n == 0) return SDSM_OK;
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hipfail(e, "hipDeviceSynchronize");
    if ((e = hipMemcpy(out, ws_words(p, d_ws)->counters, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess) return hipfail(e, "hipMemcpy");
    return SDSM_OK;
}
extern "C" double sdsm_last_solve_kernel_ms(void) { return elapsed(1, 2); }

// What the launch entry points check and prepare alike: the arguments (`outputs`: the entry point's own result pointers are all there), the
// upload, the workspace; then *P = the plan's kernel arguments in d_ws with the image pointers bound (not for an empty plan).  who: the caller's
// name in the messages; upload_hint: what it tells about a missing upload.
static int launch_front(const std::string &who, const char *upload_hint, const sdsm_plan *p, const double *const *d_y, const int32_t *const *d_atoms, const uint8_t *const *d_valid,
                        void *d_ws, size_t ws_bytes, bool outputs, BatchParams *P)
{
    if (!p || !d_y || !d_atoms || !d_valid || !d_ws || !outputs) return fail(SDSM_ERR_ARGUMENT, who + ": null argument");
    for (size_t i = 0; i < p->images.size(); i++) if (!d_y[i] || !d_atoms[i] || !d_valid[i]) return fail(SDSM_ERR_ARGUMENT, who + ": null image pointer");
    if (p->uploaded_gen != p->layout_gen || p->uploaded_ws != d_ws) return fail(SDSM_ERR_ARGUMENT, who + ": the plan's tables in this workspace are missing or stale (" + upload_hint + ")");
    if (ws_bytes < p->total) return fail(SDSM_ERR_WORKSPACE, who + ": workspace too small");
    if (p->n == 0) return SDSM_OK;
    *P = make_params(p, d_ws);
    for (size_t i = 0; i < p->images.size(); i++) { P->img[i].y = d_y[i]; P->img[i].atoms = d_atoms[i]; P->img[i].valid = d_valid[i]; }
    return SDSM_OK;
}

extern "C" int sdsm_batch_launch_multi(const sdsm_plan *p, const double *const *d_y, const int32_t *const *d_atoms, const uint8_t *const *d_valid,
                                       void *d_ws, size_t ws_bytes, sdsm_record *d_records, uint32_t *d_masks, double *d_xi, void *stream)
{
    BatchParams P;
    const int rc = launch_front("sdsm_batch_launch", "sdsm_batch_upload must follow sdsm_plan_create and every sdsm_plan_set_latency_mode", p, d_y, d_atoms, d_valid, d_ws, ws_bytes, d_records && d_masks, &P);
    if (rc != SDSM_OK || p->n == 0) return rc;
    hipError_t e;
    // the side streams of this caller stream first: a stream seen for the first time is probed (one hipStreamSynchronize of it), before any of the launch's work is queued
    LaunchStreams st{(hipStream_t)stream, {nullptr, nullptr, nullptr, nullptr}, nullptr};
    const hipStream_t s = st.caller;
    if (p->lists.forks()) {
        if ((e = acquire_sides(p, s)) != hipSuccess) return hipfail(e, "side streams (the stream must belong to the current device; a plan stays with the device of its first launch)");
        SideSet *q = p->sides;
        SideChoice c;
        std::lock_guard<std::mutex> lock(q->enqueue);
        if ((e = choose_sides(q, s, sdsm_solve_wants_own_2b(p->lists.group_members.count, p->lists.beyond_2.count) ? 4 : 3, &c)) != hipSuccess) return hipfail(e, "side streams");
        for (int i = 0; i < 4; i++) st.side[i] = c.idx[i] >= 0 ? q->pool[c.idx[i]] : nullptr;
        st.ev = q->fj;
    }
    if (g_timing && (e = hipEventRecord(g_ev[0], s)) != hipSuccess) return hipfail(e, "hipEventRecord");
    if ((e = hipMemsetAsync(ws_words(p, d_ws), 0, sizeof(LaunchWords), s)) != hipSuccess) return hipfail(e, "hipMemsetAsync");   // tickets, list heads, counters
    if ((e = sdsm_launch_setup(P, s, p->lists, p->setup_class)) != hipSuccess) return hipfail(e, "launch setup");
    if (g_timing && (e = hipEventRecord(g_ev[1], s)) != hipSuccess) return hipfail(e, "hipEventRecord");
    {
        std::unique_lock<std::mutex> enq;
        if (st.ev) enq = std::unique_lock<std::mutex>(p->sides->enqueue);
        if ((e = sdsm_launch_solve(P, SolveOutputs{d_records, d_masks, d_xi}, st, p->lists)) != hipSuccess) return hipfail(e, "launch solve");
    }
    if (g_timing) { if ((e = hipEventRecord(g_ev[2], s)) != hipSuccess) return hipfail(e, "hipEventRecord"); g_ev_valid = 1; }
    return SDSM_OK;
}

// ---- callable dsm/init (objects.py:385-386: params = init(number of columns of G~)) -----------------------------------------
// The number of columns of a candidate's G~ (its grid points, dsm.py:159-181) is known once the setup kernel has run: this runs
// it alone and returns the counts to the HOST (it synchronises the stream): n_deform[i] = M of candidate i, -1 for a candidate
// without a solve (trivial, failed setup).  The caller then builds the starting points and hands them over with sdsm_plan_set_start.
extern "C" int sdsm_batch_deform_counts(const sdsm_plan *p, const double *const *d_y, const int32_t *const *d_atoms, const uint8_t *const *d_valid,
                                        void *d_ws, size_t ws_bytes, int32_t *n_deform, void *stream)
{
    BatchParams P;
    const int rc = launch_front("sdsm_batch_deform_counts", "sdsm_batch_upload", p, d_y, d_atoms, d_valid, d_ws, ws_bytes, n_deform != nullptr, &P);
    if (rc != SDSM_OK || p->n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if ((e = sdsm_launch_setup(P, s, p->lists, p->setup_class)) != hipSuccess) return hipfail(e, "launch setup");
    std::vector<CandState> st(p->n);
    if ((e = hipMemcpyAsync(st.data(), P.state, sizeof(CandState) * p->n, hipMemcpyDeviceToHost, s)) != hipSuccess) return hipfail(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hipfail(e, "hipStreamSynchronize");
    for (int i = 0; i < p->n; i++) n_deform[i] = st[i].status == ST_OK ? (6 + st[i].M > SDSM_MAX_N_GLOBAL ? 0 : st[i].M) : -1;   // (beyond the solver's limit: elliptical model only)
    return SDSM_OK;
}

extern "C" int sdsm_batch_launch(const sdsm_plan *p, const double *d_y, const int32_t *d_atoms, const uint8_t *d_valid,
                                 void *d_ws, size_t ws_bytes, sdsm_record *d_records, uint32_t *d_masks, double *d_xi, void *stream)
{
    if (p && p->images.size() != 1) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_launch: the plan covers several images, use sdsm_batch_launch_multi");
    return sdsm_batch_launch_multi(p, &d_y, &d_atoms, &d_valid, d_ws, ws_bytes, d_records, d_masks, d_xi, stream);
}

// ---- point evaluation for parity tests ---------------------------------------------------------------------
extern "C" hipError_t sdsm_launch_eval(const BatchParams &P, const double *params, double *out, hipStream_t stream);

extern "C" int sdsm_batch_eval(const sdsm_plan *p, void *d_ws, size_t ws_bytes, const double *d_params, double *d_out, void *stream)
{
    if (!p || !d_ws || !d_params || !d_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_eval: null argument");
    if (ws_bytes < p->total) return fail(SDSM_ERR_WORKSPACE, "sdsm_batch_eval: workspace too small");
    if (p->n == 0) return SDSM_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    // results of candidates that cannot be evaluated (trivial, failed setup, beyond the solver's limits) stay NaN
    if ((e = hipMemsetAsync(d_out, 0xff, sizeof(double) * (size_t)sdsm_plan_eval_out_count(p), s)) != hipSuccess) return hipfail(e, "hipMemsetAsync");
    if (p->uploaded_gen != p->layout_gen || p->uploaded_ws != d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_eval: needs the workspace of a previous sdsm_batch_launch of this plan");
    const BatchParams P = make_params(p, d_ws);
    if ((e = sdsm_launch_eval(P, d_params, d_out, s)) != hipSuccess) return hipfail(e, "launch eval");
    return SDSM_OK;
}

// ---- one Newton step, piece by piece, in the layout of one solve class (parity tests) -----------------------
extern "C" hipError_t sdsm_launch_step_probe(const BatchParams &P, int layout, const double *params, const double *dir, double reg_mu, double tau, double t0, double *out, long long stride, hipStream_t stream);

extern "C" int sdsm_batch_eval_step(const sdsm_plan *p, void *d_ws, size_t ws_bytes, int layout, double reg_mu, double tau, double t0,
                                    const double *d_params, const double *d_dir, double *d_out, int64_t stride, void *stream)
{
    if (!p || !d_ws || !d_params || !d_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_eval_step: null argument");
    if (layout < 0 || layout >= SDSM_STEP_LAYOUT_N) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_eval_step: unknown layout");
    if (!(reg_mu >= 0 && reg_mu <= 1) || !(tau >= 0) || !(t0 > 0) || stride < SDSM_STEP_HEAD) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_eval_step: reg_mu in [0, 1], tau >= 0, t0 > 0 and stride >= SDSM_STEP_HEAD are required");
    if (ws_bytes < p->total) return fail(SDSM_ERR_WORKSPACE, "sdsm_batch_eval_step: workspace too small");
    if (p->n == 0) return SDSM_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (p->uploaded_gen != p->layout_gen || p->uploaded_ws != d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_eval_step: needs the workspace of a previous sdsm_batch_launch of this plan");
    if ((e = hipMemsetAsync(d_out, 0xff, sizeof(double) * (size_t)p->n * (size_t)stride, s)) != hipSuccess) return hipfail(e, "hipMemsetAsync");
    const BatchParams P = make_params(p, d_ws);
    if ((e = sdsm_launch_step_probe(P, layout, d_params, d_dir, reg_mu, tau, t0, d_out, (long long)stride, s)) != hipSuccess) return hipfail(e, "launch step probe");
    return SDSM_OK;
}

// ---- the scalar loss arithmetic of the solve kernels, element by element (parity tests) ---------------------
extern "C" hipError_t sdsm_launch_probe_loss(long long n, const double *y, const double *S, const double *x, double *out, hipStream_t stream);

extern "C" int sdsm_probe_loss_arithmetic(int64_t n, const double *d_y, const double *d_S, const double *d_x, double *d_out, void *stream)
{
    if (n < 0 || n > SDSM_PROBE_LOSS_MAX) return fail(SDSM_ERR_ARGUMENT, "sdsm_probe_loss_arithmetic: n out of range");
    if (n == 0) return SDSM_OK;
    if (!d_y || !d_S || !d_x || !d_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_probe_loss_arithmetic: null argument");
    hipError_t e;
    if ((e = sdsm_launch_probe_loss((long long)n, d_y, d_S, d_x, d_out, (hipStream_t)stream)) != hipSuccess) return hipfail(e, "launch probe");
    return SDSM_OK;
}

// ---- host helper: foreground fragments out of the bit-packed masks (objects.py:148-174 applied to the region-bbox masks) -------
// One byte per pixel of every fragment into `out` (fragment i: fg_h * fg_w bytes, row-major, at out_offset[i]); candidates
// without a foreground (fg_h <= 0, trivial, failed) get the single byte 0 = [[False]] (objects.py:172-174, 185-186).
// Returns the number of bytes written (or needed when out == NULL), < 0 on error.
extern "C" int64_t sdsm_unpack_fragments(const sdsm_record *records, const int32_t *mask_info, const int64_t *mask_offset, const uint8_t *masks,
                                         int n, uint8_t *out, int64_t *out_offset)
{
    if (n < 0 || (n > 0 && (!records || !mask_info || !mask_offset || !masks))) return fail(SDSM_ERR_ARGUMENT, "sdsm_unpack_fragments: null argument");
    int64_t pos = 0;
    for (int i = 0; i < n; i++) {
        const sdsm_record &r = records[i];
        const bool empty = r.fg_h <= 0 || r.status == SDSM_CAND_TRIVIAL || r.status == SDSM_CAND_ERROR || r.status == SDSM_CAND_GIVEN_UP;
        if (out_offset) out_offset[i] = pos;
        if (empty) { if (out) out[pos] = 0; pos += 1; continue; }
        const int r0 = mask_info[4 * i], c0 = mask_info[4 * i + 1], h = mask_info[4 * i + 2], w = mask_info[4 * i + 3];
        const int fr = r.fg_r0 - r0, fc = r.fg_c0 - c0;
        if (fr < 0 || fc < 0 || fr + r.fg_h > h || fc + r.fg_w > w) return fail(SDSM_ERR_ARGUMENT, "sdsm_unpack_fragments: fragment outside its mask box");
        if (out) {
            const uint32_t *words = reinterpret_cast<const uint32_t *>(masks + mask_offset[i]);
            uint8_t *o = out + pos;
            for (int a = 0; a < r.fg_h; a++) {
                int64_t bit = (int64_t)(fr + a) * w + fc;
                for (int b = 0; b < r.fg_w; b++, bit++) *o++ = (uint8_t)((words[bit >> 5] >> (bit & 31)) & 1u);
            }
        }
        pos += (int64_t)r.fg_h * r.fg_w;
    }
    return pos;
}

// ---- post-processing: the smoothed images (the per-object work, sdsm_post_objects, is with the image sets below) -------------------
extern "C" hipError_t sdsm_gaussian_filter_impl(const double *d_in, int H, int W, double sigma, double *d_out, void *d_ws, hipStream_t stream);
extern "C" size_t sdsm_gaussian_workspace_bytes(int H, int W, double sigma);

extern "C" int sdsm_gaussian_filter(const double *d_in, int H, int W, double sigma, double *d_out, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!d_in || !d_out || !d_ws || H < 1 || W < 1 || !(sigma > 0)) return fail(SDSM_ERR_ARGUMENT, "sdsm_gaussian_filter: bad argument");
    if (ws_bytes < sdsm_gaussian_workspace_bytes(H, W, sigma)) return fail(SDSM_ERR_WORKSPACE, "sdsm_gaussian_filter: workspace too small");
    hipError_t e = sdsm_gaussian_filter_impl(d_in, H, W, sigma, d_out, d_ws, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_gaussian_filter");
}

extern "C" size_t sdsm_separable_workspace_bytes(int H, int W, int R0, int R1);
extern "C" hipError_t sdsm_separable_filter_impl(const double *d_in, int H, int W, const double *h_w0, int R0, const double *h_w1, int R1,
                                                 double *d_out, void *d_ws, hipStream_t stream);
extern "C" int sdsm_separable_filter(const double *d_in, int H, int W, const double *h_w0, int R0, const double *h_w1, int R1,
                                     double *d_out, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!d_in || !d_out || !d_ws || !h_w0 || !h_w1 || H < 1 || W < 1 || R0 < 0 || R1 < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_separable_filter: bad argument");
    for (int j = 1; j <= R0; j++) if (h_w0[R0 - j] != h_w0[R0 + j]) return fail(SDSM_ERR_ARGUMENT, "sdsm_separable_filter: weights must be symmetric");
    for (int j = 1; j <= R1; j++) if (h_w1[R1 - j] != h_w1[R1 + j]) return fail(SDSM_ERR_ARGUMENT, "sdsm_separable_filter: weights must be symmetric");
    if (ws_bytes < sdsm_separable_workspace_bytes(H, W, R0, R1)) return fail(SDSM_ERR_WORKSPACE, "sdsm_separable_filter: workspace too small");
    hipError_t e = sdsm_separable_filter_impl(d_in, H, W, h_w0, R0, h_w1, R1, d_out, d_ws, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_separable_filter (the LDS tiles take a filter radius of at most 1240 for the column pass and 10048 for the row pass)");
}

// ---- scale estimation (automation.py:13-68): LoG masks, integral image, determinant-of-Hessian cube, peaks ----
extern "C" hipError_t sdsm_log_masks_impl(const double *d_im, int H, int W, int n_scales, const int32_t *h_radii, const double *d_weights,
                                          uint8_t *d_masks, void *d_ws, hipStream_t stream);
extern "C" hipError_t sdsm_integral_image_impl(const double *d_im, int H, int W, double *d_ii, hipStream_t stream);
extern "C" hipError_t sdsm_doh_cube_impl(const double *d_ii, int H, int W, int n_scales, const int32_t *h_box, const double *h_w_i,
                                         const uint8_t *d_masks, double *d_cube, hipStream_t stream);
extern "C" hipError_t sdsm_doh_peaks_impl(const double *d_cube, int H, int W, int n_scales, double threshold, void *d_out, int64_t capacity,
                                          hipStream_t stream);

extern "C" int sdsm_log_masks(const double *d_im, int H, int W, int n_scales, const int32_t *h_radii, const double *d_weights, uint8_t *d_masks,
                              void *d_ws, size_t ws_bytes, void *stream)
{
    if (!d_im || !d_weights || !d_masks || !d_ws || !h_radii || H < 1 || W < 1 || n_scales < 1) return fail(SDSM_ERR_ARGUMENT, "sdsm_log_masks: bad argument");
    for (int s = 0; s < n_scales; s++) if (h_radii[s] < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_log_masks: negative radius");
    if (ws_bytes < sdsm_log_masks_workspace_bytes(H, W)) return fail(SDSM_ERR_WORKSPACE, "sdsm_log_masks: workspace too small");
    hipError_t e = sdsm_log_masks_impl(d_im, H, W, n_scales, h_radii, d_weights, d_masks, d_ws, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_log_masks (radii as sdsm_separable_filter takes them)");
}

extern "C" int sdsm_integral_image(const double *d_im, int H, int W, double *d_ii, void *stream)
{
    if (!d_im || !d_ii || H < 1 || W < 1) return fail(SDSM_ERR_ARGUMENT, "sdsm_integral_image: bad argument");
    hipError_t e = sdsm_integral_image_impl(d_im, H, W, d_ii, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_integral_image");
}

extern "C" int sdsm_doh_cube(const double *d_ii, int H, int W, int n_scales, const int32_t *h_box, const double *h_w_i, const uint8_t *d_masks,
                             double *d_cube, void *stream)
{
    if (!d_ii || !h_box || !h_w_i || !d_cube || H < 1 || W < 1 || n_scales < 1 || n_scales > SDSM_DOH_MAX_SCALES || H > 65535)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_doh_cube: bad argument");
    for (int s = 0; s < n_scales; s++) {
        const int32_t *b = h_box + 3 * s;
        if (b[0] < 1 || b[0] > (1 << 24) || b[1] < 0 || b[2] < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_doh_cube: bad box sizes");
    }
    hipError_t e = sdsm_doh_cube_impl(d_ii, H, W, n_scales, h_box, h_w_i, d_masks, d_cube, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_doh_cube");
}

extern "C" int sdsm_doh_peaks(const double *d_cube, int H, int W, int n_scales, double threshold, void *d_out, int64_t capacity, void *stream)
{
    if (!d_cube || !d_out || H < 1 || W < 1 || n_scales < 1 || capacity < 0 || H > 65535) return fail(SDSM_ERR_ARGUMENT, "sdsm_doh_peaks: bad argument");
    hipError_t e = sdsm_doh_peaks_impl(d_cube, H, W, n_scales, threshold, d_out, capacity, (hipStream_t)stream);
    return e == hipSuccess ? SDSM_OK : hipfail(e, "sdsm_doh_peaks");
}

// ---- image sets: C2F markers, exact EDT, per-object post-processing (a single image is the set of one) -------------------------------
extern "C" size_t sdsm_c2f_markers_workspace_bytes_multi_impl(const sdsm_set_image *images, int n_images);
extern "C" hipError_t sdsm_c2f_markers_multi_impl(const sdsm_set_image *images, int n_images, const double *d_y, const double *thr,
                                                  uint8_t *d_y_mask, int32_t *d_markers, int32_t *d_count, void *d_ws, hipStream_t stream);
extern "C" size_t sdsm_edt_exact_workspace_bytes_multi_impl(const sdsm_set_image *images, int n_images);
extern "C" hipError_t sdsm_edt_exact_multi_impl(const sdsm_set_image *images, int n_images, const uint8_t *d_target, double *d_out, void *d_ws,
                                                hipStream_t stream);
extern "C" hipError_t sdsm_launch_post_set(const sdsm_post_image *images, int n_images, const int32_t *boxes, const int64_t *bits_off,
                                           const uint32_t *bits, const int64_t *new_off, uint32_t *new_bits, uint32_t *boundary_pool,
                                           const int64_t *bpool_off, double exterior_scale, double exterior_offset, double contrast_epsilon,
                                           int max_distance, double stdamp, sdsm_post_record *out, hipStream_t stream);
extern "C" hipError_t sdsm_launch_post_background(const sdsm_post_bg_image *images, int n_images, const int32_t *boxes, const int64_t *bits_off,
                                                  const uint32_t *bits, int radius, hipStream_t stream);
extern "C" hipError_t sdsm_launch_post_fill(int n, const int32_t *dims, const int64_t *off, const uint32_t *in, uint32_t *out, uint32_t *ws,
                                            const int64_t *ws_off, int32_t *status, hipStream_t stream);
extern "C" hipError_t sdsm_launch_post_glare(const sdsm_post_image *images, int n_images, const int32_t *boxes, const int64_t *bits_off,
                                             const uint32_t *bits, const double *props, int num_layers, uint32_t *ws, const int64_t *ws_off,
                                             int32_t *out, hipStream_t stream);

// The table of a set: 1 .. SDSM_MAX_SET_IMAGES images, offsets >= 0, H, W >= 1, and the limits of the kernels that take it.
enum { SET_PIXELS = 1,      // H * W < 2^31: pixel indices are int32
       SET_SIDES = 2 };     // H, W <= 65535: coordinates packed into 16 bits, squared distances in int64
static int64_t set_offset(const sdsm_set_image &im) { return im.offset; }
static int64_t set_offset(const sdsm_post_image &) { return 0; }      // (its images are not packed: device pointers)
static int64_t set_offset(const sdsm_post_bg_image &) { return 0; }
template <class Image> static bool set_table_ok(const Image *images, int n_images, int limits)
{
    if (!images || n_images < 1 || n_images > SDSM_MAX_SET_IMAGES) return false;
    for (int i = 0; i < n_images; i++) {
        const Image &im = images[i];
        if (set_offset(im) < 0 || im.H < 1 || im.W < 1) return false;
        if ((limits & SET_PIXELS) && (int64_t)im.H * im.W >= INT_MAX) return false;
        if ((limits & SET_SIDES) && (im.H > 65535 || im.W > 65535)) return false;
    }
    return true;
}
#define SET_TABLE(name, limits) \
    if (!set_table_ok(images, n_images, limits)) \
        return fail(SDSM_ERR_ARGUMENT, std::string(name ": bad image table (1 .. 32 images, offset >= 0, 1 <= H, W") + \
                                       ((limits) & SET_SIDES ? " <= 65535" : "") + ((limits) & SET_PIXELS ? ", H * W < 2^31)" : ")"))
#define SET_DONE(name) return e == hipSuccess ? SDSM_OK : hipfail(e, name)

// H^2 + W^2 < 2^31: every squared distance fits int32 (and so every side 16 bits, H * W 30 bits)
static bool boundary_shapes_ok(const sdsm_set_image *images, int n_images)
{
    for (int i = 0; i < n_images; i++)
        if ((int64_t)images[i].H * images[i].H + (int64_t)images[i].W * images[i].W >= (int64_t)1 << 31) return false;
    return true;
}

// The ranges [off[i], off[i] + len[i]) that the images of a set own in a shared buffer.  The walk goes image by image: image i's own range
// (len_ok, off >= 0), then its overlap with every image j before it.  Where it stops, *why is what the message says behind the entry's name
// and *at a number that grows along the walk, so that an entry with two tables (sdsm_neighbours) reports what comes first.
template <class Len, class Ok>
static bool ranges_ok(int n_images, const int64_t *off, const Len *len, Ok len_ok, bool check_overlap, const char *bad_range, const char *overlap,
                      const char **why, int *at)
{
    for (int i = 0; i < n_images; i++) {
        if (!len_ok(len[i]) || off[i] < 0) { *why = bad_range; if (at) *at = i * (SDSM_MAX_SET_IMAGES + 1); return false; }
        for (int j = 0; check_overlap && j < i; j++)
            if (off[i] < off[j] + len[j] && off[j] < off[i] + len[i]) { *why = overlap; if (at) *at = i * (SDSM_MAX_SET_IMAGES + 1) + j + 1; return false; }
    }
    return true;
}

// the label records of a set: n_labels[i] records from rec_off[i] on
static bool label_records_ok(int n_images, const int32_t *n_labels, const int64_t *rec_off, bool check_overlap, const char **why, int *at = nullptr)
{
    return ranges_ok(n_images, rec_off, n_labels, [](int32_t n) { return n >= 1 && n <= SDSM_MEASURE_MAX_LABELS; }, check_overlap,
                     "1 <= n_labels <= 65536 and rec_off >= 0 required", "the records of two images overlap", why, at);
}

// the pair tables of a set: capacity[i] slots from table_off[i] on
static bool pair_tables_ok(int n_images, const int64_t *table_off, const int64_t *capacity, const char **why, int *at = nullptr)
{
    return ranges_ok(n_images, table_off, capacity, [](int64_t c) { return c >= 1 && (c & (c - 1)) == 0; }, true,
                     "capacity a power of two >= 1 and table_off >= 0 required", "the tables of two images overlap", why, at);
}

extern "C" size_t sdsm_c2f_markers_workspace_bytes_multi(const sdsm_set_image *images, int n_images)
{
    return set_table_ok(images, n_images, SET_PIXELS) ? sdsm_c2f_markers_workspace_bytes_multi_impl(images, n_images) : 0;
}

extern "C" int sdsm_c2f_markers_multi(const sdsm_set_image *images, int n_images, const double *d_y, const double *max_irregularity,
                                      uint8_t *d_y_mask, int32_t *d_markers, int32_t *d_count, void *d_ws, size_t ws_bytes, void *stream)
{
    SET_TABLE("sdsm_c2f_markers_multi", SET_PIXELS);
    if (!d_y || !max_irregularity || !d_y_mask || !d_markers || !d_count || !d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_c2f_markers_multi: null argument");
    if (ws_bytes < sdsm_c2f_markers_workspace_bytes_multi_impl(images, n_images)) return fail(SDSM_ERR_WORKSPACE, "sdsm_c2f_markers_multi: workspace too small");
    hipError_t e = sdsm_c2f_markers_multi_impl(images, n_images, d_y, max_irregularity, d_y_mask, d_markers, d_count, d_ws, (hipStream_t)stream);
    SET_DONE("sdsm_c2f_markers_multi");
}

// (the single-image queries answer for every H, W >= 1, also where the call itself refuses the shape)
extern "C" size_t sdsm_c2f_markers_workspace_bytes(int H, int W)
{
    const sdsm_set_image one = {0, H, W};
    return H < 1 || W < 1 ? 0 : sdsm_c2f_markers_workspace_bytes_multi_impl(&one, 1);
}

extern "C" int sdsm_c2f_markers(const double *d_y, int H, int W, double max_irregularity, uint8_t *d_y_mask, int32_t *d_markers, int32_t *d_count,
                                void *d_ws, size_t ws_bytes, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_c2f_markers_multi(&one, 1, d_y, &max_irregularity, d_y_mask, d_markers, d_count, d_ws, ws_bytes, stream);
}

extern "C" size_t sdsm_edt_exact_workspace_bytes_multi(const sdsm_set_image *images, int n_images)
{
    return set_table_ok(images, n_images, SET_SIDES) ? sdsm_edt_exact_workspace_bytes_multi_impl(images, n_images) : 0;
}

extern "C" int sdsm_edt_exact_multi(const sdsm_set_image *images, int n_images, const uint8_t *d_target, double *d_out, void *d_ws, size_t ws_bytes,
                                    void *stream)
{
    SET_TABLE("sdsm_edt_exact_multi", SET_SIDES);
    if (!d_target || !d_out || !d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_edt_exact_multi: null argument");
    if (ws_bytes < sdsm_edt_exact_workspace_bytes_multi_impl(images, n_images)) return fail(SDSM_ERR_WORKSPACE, "sdsm_edt_exact_multi: workspace too small");
    hipError_t e = sdsm_edt_exact_multi_impl(images, n_images, d_target, d_out, d_ws, (hipStream_t)stream);
    SET_DONE("sdsm_edt_exact_multi");
}

extern "C" size_t sdsm_edt_exact_workspace_bytes(int H, int W)
{
    const sdsm_set_image one = {0, H, W};
    return H < 1 || W < 1 ? 0 : sdsm_edt_exact_workspace_bytes_multi_impl(&one, 1);
}

extern "C" int sdsm_edt_exact(const uint8_t *d_target, int H, int W, double *d_out, void *d_ws, size_t ws_bytes, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_edt_exact_multi(&one, 1, d_target, d_out, d_ws, ws_bytes, stream);
}

extern "C" int sdsm_post_objects_multi(const sdsm_post_image *images, int n_images, const int32_t *d_boxes, const int64_t *d_bits_off,
                                       const uint32_t *d_bits, const int64_t *d_new_off, uint32_t *d_new_bits, uint32_t *d_boundary_pool,
                                       const int64_t *d_bpool_off, double exterior_scale, double exterior_offset, double contrast_epsilon,
                                       int max_distance, double stdamp, sdsm_post_record *d_out, void *stream)
{
    SET_TABLE("sdsm_post_objects_multi", SET_SIDES);
    int64_t n = 0;
    for (int j = 0; j < n_images; j++) {
        const sdsm_post_image &im = images[j];
        if (im.n_objects < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: negative object count");
        if (im.n_objects > 0 && (!im.d_g || !im.d_gs || !im.d_bg)) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: null image input");
        n += im.n_objects;
    }
    if (n >= INT_MAX) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: more than 2^31 - 1 objects");
    if (n == 0) return SDSM_OK;
    if (!d_boxes || !d_bits_off || !d_bits || !d_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: null argument");
    if (!(exterior_scale > 0) || !(exterior_offset >= 0) || max_distance < 0 || max_distance > 16) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: exterior_scale > 0, exterior_offset >= 0, 0 <= max_distance <= 16 required");
    if (max_distance > 0 && stdamp > 0 && (!d_new_off || !d_new_bits)) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: refinement needs the output mask buffers");
    if ((d_boundary_pool == nullptr) != (d_bpool_off == nullptr)) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_objects_multi: boundary pool and its offsets go together");
    hipError_t e = sdsm_launch_post_set(images, n_images, d_boxes, d_bits_off, d_bits, d_new_off, d_new_bits, d_boundary_pool, d_bpool_off,
                                        exterior_scale, exterior_offset, contrast_epsilon, max_distance, stdamp, d_out, (hipStream_t)stream);
    SET_DONE("sdsm_post_objects_multi");
}

extern "C" int sdsm_post_objects(const double *d_g, const double *d_gs, const uint8_t *d_bg, int H, int W, int n, const int32_t *d_boxes,
                                 const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_new_off, uint32_t *d_new_bits,
                                 uint32_t *d_boundary_pool, const int64_t *d_bpool_off, double exterior_scale, double exterior_offset,
                                 double contrast_epsilon, double inv_gstd, int max_distance, double stdamp, sdsm_post_record *d_out, void *stream)
{
    const sdsm_post_image one = {d_g, d_gs, d_bg, H, W, inv_gstd, n, 0};
    return sdsm_post_objects_multi(&one, 1, d_boxes, d_bits_off, d_bits, d_new_off, d_new_bits, d_boundary_pool, d_bpool_off, exterior_scale,
                                   exterior_offset, contrast_epsilon, max_distance, stdamp, d_out, stream);
}

// ---- label maps and overlays (sdsm_render.hip) -----------------------------------------------------------------------------------
extern "C" hipError_t sdsm_render_morph_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                             const int64_t *bits_off, const uint32_t *bits, int radius, const int64_t *new_off, uint32_t *new_bits,
                                             int32_t *area, hipStream_t stream);
extern "C" hipError_t sdsm_render_overlaps_impl(int n_pairs, const int32_t *pairs, const int32_t *boxes, const int64_t *bits_off, const uint32_t *bits,
                                                int32_t *inter, hipStream_t stream);
extern "C" hipError_t sdsm_render_paint_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                             const int64_t *bits_off, const uint32_t *bits, const int32_t *obj_label, int32_t *label, uint8_t *cover,
                                             uint8_t *target, hipStream_t stream);
extern "C" hipError_t sdsm_render_lost_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                            const int64_t *bits_off, const uint32_t *bits, const int32_t *obj_label, int32_t *label, int32_t *lost,
                                            int n_labels, int32_t *vmax, hipStream_t stream);
extern "C" hipError_t sdsm_render_fill_impl(const sdsm_set_image *images, int n_images, int n_sel, const int32_t *sel, const int32_t *obj_image,
                                            const int32_t *boxes, const int64_t *bits_off, const uint32_t *bits, const int32_t *obj_label,
                                            int32_t new_label, int32_t *label, int32_t *filled, hipStream_t stream);
extern "C" hipError_t sdsm_render_compact_impl(const sdsm_set_image *images, int n_images, const int32_t *label, const uint8_t *cover, const double *dist,
                                               const int64_t *capacity, void *entries, int32_t *counts, hipStream_t stream);
extern "C" hipError_t sdsm_render_scatter_impl(int64_t n, const int64_t *pix, const int32_t *lab, int32_t *label, hipStream_t stream);
extern "C" hipError_t sdsm_render_finish_impl(int64_t n, const int32_t *label, uint16_t bg, uint16_t *out, hipStream_t stream);
extern "C" hipError_t sdsm_render_overlay_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const double *base, int channels,
                                               int kind, int radius, const double *color, const double *bg, int has_bg, int background_label,
                                               uint8_t *out, hipStream_t stream);

extern "C" int sdsm_render_morph_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                       const int64_t *d_bits_off, const uint32_t *d_bits, int radius, const int64_t *d_new_off, uint32_t *d_new_bits,
                                       int32_t *d_area, void *stream)
{
    SET_TABLE("sdsm_render_morph", SET_SIDES | SET_PIXELS);
    if (radius == 0 || radius > SDSM_RENDER_MAX_RADIUS || radius < -SDSM_RENDER_MAX_RADIUS)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_morph: 1 <= |radius| <= 16 required");
    if (n < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_morph: n < 0");
    if (n == 0) return SDSM_OK;
    if (!d_boxes || !d_bits_off || !d_bits || !d_new_off || !d_new_bits || !d_area || (n_images > 1 && !d_obj_image))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_morph: null argument");
    hipError_t e = sdsm_render_morph_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, radius, d_new_off, d_new_bits, d_area, (hipStream_t)stream);
    SET_DONE("sdsm_render_morph");
}

extern "C" int sdsm_render_morph(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, int radius,
                                 const int64_t *d_new_off, uint32_t *d_new_bits, int32_t *d_area, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_morph_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, radius, d_new_off, d_new_bits, d_area, stream);
}

extern "C" int sdsm_render_overlaps(int n_pairs, const int32_t *d_pairs, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits,
                                    int32_t *d_inter, void *stream)
{
    if (n_pairs < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_overlaps: n_pairs < 0");
    if (n_pairs == 0) return SDSM_OK;
    if (!d_pairs || !d_boxes || !d_bits_off || !d_bits || !d_inter) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_overlaps: null argument");
    hipError_t e = sdsm_render_overlaps_impl(n_pairs, d_pairs, d_boxes, d_bits_off, d_bits, d_inter, (hipStream_t)stream);
    SET_DONE("sdsm_render_overlaps");
}

extern "C" int sdsm_render_paint_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                       const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label, int32_t *d_label,
                                       uint8_t *d_cover, uint8_t *d_target, void *stream)
{
    SET_TABLE("sdsm_render_paint", SET_SIDES | SET_PIXELS);
    if (n < 0 || !d_label || !d_cover || !d_target) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_paint: bad argument");
    if (n > 0 && (!d_boxes || !d_bits_off || !d_bits || !d_obj_label || (n_images > 1 && !d_obj_image)))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_paint: null argument");
    hipError_t e = sdsm_render_paint_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_obj_label, d_label, d_cover, d_target, (hipStream_t)stream);
    SET_DONE("sdsm_render_paint");
}

extern "C" int sdsm_render_paint(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits,
                                 const int32_t *d_obj_label, int32_t *d_label, uint8_t *d_cover, uint8_t *d_target, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_paint_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_obj_label, d_label, d_cover, d_target, stream);
}

extern "C" int sdsm_render_compact_multi(const sdsm_set_image *images, int n_images, const int32_t *d_label, const uint8_t *d_cover, const double *d_dist,
                                         const int64_t *capacity, sdsm_render_entry *d_entries, int32_t *d_counts, void *stream)
{
    SET_TABLE("sdsm_render_compact", SET_SIDES | SET_PIXELS);
    if (!d_label || !d_cover || !d_dist || !capacity || !d_entries || !d_counts) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_compact: null argument");
    for (int i = 0; i < n_images; i++) if (capacity[i] < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_compact: negative capacity");
    hipError_t e = sdsm_render_compact_impl(images, n_images, d_label, d_cover, d_dist, capacity, d_entries, d_counts, (hipStream_t)stream);
    SET_DONE("sdsm_render_compact");
}

extern "C" int sdsm_render_compact(int H, int W, const int32_t *d_label, const uint8_t *d_cover, const double *d_dist, int64_t capacity,
                                   sdsm_render_entry *d_entries, int32_t *d_count, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_compact_multi(&one, 1, d_label, d_cover, d_dist, &capacity, d_entries, d_count, stream);
}

extern "C" int sdsm_render_scatter(int64_t n, const int64_t *d_pix, const int32_t *d_lab, int32_t *d_label, void *stream)
{
    if (n < 0 || n >= ((int64_t)INT_MAX - 1) * 256) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_scatter: bad count");
    if (n == 0) return SDSM_OK;
    if (!d_pix || !d_lab || !d_label) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_scatter: null argument");
    hipError_t e = sdsm_render_scatter_impl(n, d_pix, d_lab, d_label, (hipStream_t)stream);
    SET_DONE("sdsm_render_scatter");
}

extern "C" int sdsm_render_lost_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                      const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label, int n_labels, int32_t *d_label,
                                      int32_t *d_lost, int32_t *d_max, void *stream)
{
    SET_TABLE("sdsm_render_lost", SET_SIDES | SET_PIXELS);
    if (n < 1 || n_labels < 1 || !d_boxes || !d_bits_off || !d_bits || !d_obj_label || !d_label || !d_lost || !d_max || (n_images > 1 && !d_obj_image))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_lost: bad argument");
    hipError_t e = sdsm_render_lost_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_obj_label, d_label, d_lost, n_labels, d_max, (hipStream_t)stream);
    SET_DONE("sdsm_render_lost");
}

extern "C" int sdsm_render_lost(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label,
                                int n_labels, int32_t *d_label, int32_t *d_lost, int32_t *d_max, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_lost_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_obj_label, n_labels, d_label, d_lost, d_max, stream);
}

extern "C" int sdsm_render_fill_multi(const sdsm_set_image *images, int n_images, int n_sel, const int32_t *d_sel, const int32_t *d_obj_image,
                                      const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int32_t *d_obj_label,
                                      int new_label, int32_t *d_label, int32_t *d_filled, void *stream)
{
    SET_TABLE("sdsm_render_fill", SET_SIDES | SET_PIXELS);
    if (n_sel < 1 || new_label < 1 || new_label > 65535 || !d_sel || !d_boxes || !d_bits_off || !d_bits || !d_obj_label || !d_label || !d_filled || (n_images > 1 && !d_obj_image))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_fill: bad argument (1 <= new_label <= 65535)");
    hipError_t e = sdsm_render_fill_impl(images, n_images, n_sel, d_sel, d_obj_image, d_boxes, d_bits_off, d_bits, d_obj_label, new_label, d_label, d_filled, (hipStream_t)stream);
    SET_DONE("sdsm_render_fill");
}

extern "C" int sdsm_render_fill(int H, int W, int n_sel, const int32_t *d_sel, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits,
                                const int32_t *d_obj_label, int new_label, int32_t *d_label, int32_t *d_filled, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_fill_multi(&one, 1, n_sel, d_sel, nullptr, d_boxes, d_bits_off, d_bits, d_obj_label, new_label, d_label, d_filled, stream);
}

extern "C" int sdsm_render_finish(int64_t n, const int32_t *d_label, int background_label, uint16_t *d_out, void *stream)
{
    if (n < 1 || n >= ((int64_t)INT_MAX - 1) * 256 || !d_label || !d_out || background_label > 0 || background_label < -65535)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_finish: bad argument (-65535 <= background_label <= 0)");
    hipError_t e = sdsm_render_finish_impl(n, d_label, (uint16_t)background_label, d_out, (hipStream_t)stream);
    SET_DONE("sdsm_render_finish");
}

extern "C" int sdsm_render_overlay_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const double *d_base, int channels,
                                         int kind, int radius, const double *color, const double *bg, int background_label, uint8_t *d_out, void *stream)
{
    SET_TABLE("sdsm_render_overlay", SET_SIDES | SET_PIXELS);
    if (radius < 0 || radius > SDSM_RENDER_MAX_RADIUS) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_overlay: 0 <= radius <= 16 required");
    if (kind < 0 || kind > 3 || !d_labels || !d_out || (kind != 3 && ((channels != 1 && channels != 3) || !color || !d_base)))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_overlay: bad argument (kind 0 .. 3, channels 1 or 3)");
    static const double no_color[3] = {0, 0, 0};
    if (!color) color = no_color;
    hipError_t e = sdsm_render_overlay_impl(images, n_images, d_labels, d_base, channels, kind, radius, color, bg, bg != nullptr, background_label, d_out, (hipStream_t)stream);
    SET_DONE("sdsm_render_overlay");
}

extern "C" int sdsm_render_overlay(int H, int W, const int32_t *d_labels, const double *d_base, int channels, int kind, int radius, const double *color,
                                   const double *bg, int background_label, uint8_t *d_out, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_overlay_multi(&one, 1, d_labels, d_base, channels, kind, radius, color, bg, background_label, d_out, stream);
}

// ---- colour maps and adjacency graphs (sdsm_render.hip) ----------------------------------------------------------------------------
extern "C" hipError_t sdsm_render_label_range_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int32_t *perm,
                                                   const int64_t *perm_off, const int32_t *perm_min, int32_t *range, int32_t *permuted_out,
                                                   hipStream_t stream);
extern "C" hipError_t sdsm_render_colormap_impl(const sdsm_set_image *images, int n_images, int source, const void *src, const double *lut, int N,
                                                const double *clim, const int32_t *perm, const int64_t *perm_off, const int32_t *perm_min,
                                                const int32_t *range, int has_bg, int bg_label, const double *bg_color, int32_t *flags,
                                                double *out, hipStream_t stream);
extern "C" hipError_t sdsm_render_graph_impl(const sdsm_set_image *images, int n_images, int n_prims, const int32_t *prims, double rim_radius,
                                             double disk_radius, int seed_reach, int line_reach, int core_d2, int ring_d2, const double *colors,
                                             const double *base, int channels, int32_t *key, uint8_t *out, hipStream_t stream);

static bool perm_tables_ok(int n_images, const int32_t *d_perm, const int64_t *perm_off, const int32_t *perm_min)
{
    if (!d_perm) return true;
    if (!perm_off || !perm_min || perm_off[0] < 0) return false;
    for (int i = 0; i < n_images; i++) if (perm_off[i + 1] < perm_off[i]) return false;
    return true;
}

extern "C" int sdsm_render_label_range_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_perm,
                                             const int64_t *perm_off, const int32_t *perm_min, int32_t *d_range, int32_t *d_permuted, void *stream)
{
    SET_TABLE("sdsm_render_label_range", SET_SIDES | SET_PIXELS);
    if (!d_labels || (!d_range && !d_permuted)) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_label_range: null argument");
    if (!perm_tables_ok(n_images, d_perm, perm_off, perm_min)) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_label_range: bad permutation tables");
    hipError_t e = sdsm_render_label_range_impl(images, n_images, d_labels, d_perm, perm_off, perm_min, d_range, d_permuted, (hipStream_t)stream);
    SET_DONE("sdsm_render_label_range");
}

extern "C" int sdsm_render_label_range(int H, int W, const int32_t *d_labels, const int32_t *d_perm, int64_t perm_n, int perm_min, int32_t *d_range,
                                       int32_t *d_permuted, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off[2] = {0, perm_n};
    return sdsm_render_label_range_multi(&one, 1, d_labels, d_perm, off, &perm_min, d_range, d_permuted, stream);
}

extern "C" int sdsm_render_colormap_multi(const sdsm_set_image *images, int n_images, int source, const void *d_src, const double *d_lut, int N,
                                          const double *clim, const int32_t *d_perm, const int64_t *perm_off, const int32_t *perm_min,
                                          const int32_t *d_range, const double *bg_color, int bg_label, int32_t *d_flags, double *d_out, void *stream)
{
    SET_TABLE("sdsm_render_colormap", SET_SIDES | SET_PIXELS);
    if (N < 1 || N > SDSM_RENDER_MAX_COLORS) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_colormap: 1 <= N <= 1024 colours required");
    if ((source != 0 && source != 1) || !d_src || !d_lut || !d_out || (source == 0 && (!clim || !d_flags)) || (source == 1 && !d_range))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_colormap: bad argument (source 0 needs clim and d_flags, source 1 d_range)");
    if (source == 1 && !perm_tables_ok(n_images, d_perm, perm_off, perm_min)) return fail(SDSM_ERR_ARGUMENT, "sdsm_render_colormap: bad permutation tables");
    hipError_t e = sdsm_render_colormap_impl(images, n_images, source, d_src, d_lut, N, clim, source == 1 ? d_perm : nullptr, perm_off, perm_min, d_range,
                                             bg_color != nullptr, bg_label, bg_color, d_flags, d_out, (hipStream_t)stream);
    SET_DONE("sdsm_render_colormap");
}

extern "C" int sdsm_render_colormap(int H, int W, int source, const void *d_src, const double *d_lut, int N, const double *clim, const int32_t *d_perm,
                                    int64_t perm_n, int perm_min, const int32_t *d_range, const double *bg_color, int bg_label, int32_t *d_flags,
                                    double *d_out, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off[2] = {0, perm_n};
    return sdsm_render_colormap_multi(&one, 1, source, d_src, d_lut, N, clim, d_perm, off, &perm_min, d_range, bg_color, bg_label, d_flags, d_out, stream);
}

extern "C" int sdsm_render_graph_multi(const sdsm_set_image *images, int n_images, int n_prims, const int32_t *d_prims, double rim_radius,
                                       double disk_radius, int line_reach, int core_d2, int ring_d2, const double *colors, const double *d_base,
                                       int channels, int32_t *d_key, uint8_t *d_out, void *stream)
{
    SET_TABLE("sdsm_render_graph", SET_SIDES | SET_PIXELS);
    if (!(rim_radius >= 0) || !(disk_radius >= 0) || rim_radius > SDSM_RENDER_MAX_SEED_RADIUS || disk_radius > SDSM_RENDER_MAX_SEED_RADIUS)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_graph: 0 <= radius <= 64 required for the disks and their rims");
    if (line_reach < 0 || line_reach > SDSM_RENDER_MAX_RADIUS || core_d2 < -1 || ring_d2 < core_d2 || (int64_t)ring_d2 >= (int64_t)(line_reach + 1) * (line_reach + 1))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_graph: bad line (0 <= line_reach <= 16, -1 <= core_d2 <= ring_d2 < (line_reach + 1)^2)");
    if (n_prims < 0 || (n_prims > 0 && !d_prims) || !colors || !d_base || (channels != 1 && channels != 3) || !d_key || !d_out)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_render_graph: bad argument (channels 1 or 3)");
    const double reach = rim_radius > disk_radius ? rim_radius : disk_radius;
    hipError_t e = sdsm_render_graph_impl(images, n_images, n_prims, d_prims, rim_radius, disk_radius, (int)ceil(reach), line_reach, core_d2, ring_d2, colors,
                                          d_base, channels, d_key, d_out, (hipStream_t)stream);
    SET_DONE("sdsm_render_graph");
}

extern "C" int sdsm_render_graph(int H, int W, int n_prims, const int32_t *d_prims, double rim_radius, double disk_radius, int line_reach, int core_d2,
                                 int ring_d2, const double *colors, const double *d_base, int channels, int32_t *d_key, uint8_t *d_out, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_render_graph_multi(&one, 1, n_prims, d_prims, rim_radius, disk_radius, line_reach, core_d2, ring_d2, colors, d_base, channels, d_key, d_out, stream);
}

// ---- per-object measurement tables (sdsm_measure.hip) ------------------------------------------------------------------------------
extern "C" hipError_t sdsm_measure_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                const int64_t *bits_off, const uint32_t *bits, const double *d_g, double *d_gmax_abs,
                                                int32_t *d_scale_exp, sdsm_measure_record *out, hipStream_t stream);
extern "C" hipError_t sdsm_measure_labels_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int64_t *rec_off,
                                               const int32_t *n_labels, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                               sdsm_measure_record *out, int32_t *bad, hipStream_t stream);

// the packed objects of a call, as the nine table entries below take them: n boxes, the offsets of their words and the words, and the image of every
// object where the set has more than one; null: fine
static const char *packed_objects_bad(int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                                      const uint32_t *d_bits)
{
    if (n < 0) return "n < 0";
    if (n > 0 && (!d_boxes || !d_bits_off || !d_bits || (n_images > 1 && !d_obj_image))) return "null argument";
    return nullptr;
}

extern "C" int sdsm_measure_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                          const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, double *d_gmax_abs,
                                          int32_t *d_scale_exp, sdsm_measure_record *d_out, void *stream)
{
    SET_TABLE("sdsm_measure_objects", SET_SIDES | SET_PIXELS);
    if (const char *why = packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits))
        return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_measure_objects: ") + why);
    if (d_g && !d_gmax_abs) return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_objects: intensities need d_gmax_abs");
    if (n > 0 && !d_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_objects: null argument");
    hipError_t e = sdsm_measure_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, d_gmax_abs, d_scale_exp, d_out,
                                             (hipStream_t)stream);
    SET_DONE("sdsm_measure_objects");
}

extern "C" int sdsm_measure_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                                    double *d_gmax_abs, int32_t *d_scale_exp, sdsm_measure_record *d_out, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_measure_objects_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_g, d_gmax_abs, d_scale_exp, d_out, stream);
}

extern "C" int sdsm_measure_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off,
                                         const int32_t *n_labels, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                         sdsm_measure_record *d_out, int32_t *d_bad, void *stream)
{
    SET_TABLE("sdsm_measure_labels", SET_SIDES | SET_PIXELS);
    if (!d_labels || !rec_off || !n_labels || !d_out || !d_bad) return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_labels: null argument");
    if (d_g && !d_gmax_abs) return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_labels: intensities need d_gmax_abs");
    const char *why;
    if (!label_records_ok(n_images, n_labels, rec_off, true, &why)) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_measure_labels: ") + why);
    hipError_t e = sdsm_measure_labels_impl(images, n_images, d_labels, rec_off, n_labels, d_g, d_gmax_abs, d_scale_exp, d_out, d_bad, (hipStream_t)stream);
    SET_DONE("sdsm_measure_labels");
}

extern "C" int sdsm_measure_labels(int H, int W, const int32_t *d_labels, int n_labels, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                   sdsm_measure_record *d_out, int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_measure_labels_multi(&one, 1, d_labels, &off, &n_labels, d_g, d_gmax_abs, d_scale_exp, d_out, d_bad, stream);
}

// ---- contour shape tables (sdsm_shape.hip) ----------------------------------------------------------------------------------------------
extern "C" hipError_t sdsm_shape_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                              const int64_t *bits_off, const uint32_t *bits, const int64_t *slot_off, int32_t *slots,
                                              sdsm_shape_record *out, int64_t *vert_off, int32_t *verts, hipStream_t stream);
extern "C" hipError_t sdsm_shape_scatter_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int64_t *rec_off,
                                              const int32_t *n_labels, const int32_t *label_obj, int n, const int32_t *boxes, const int64_t *bits_off,
                                              int64_t window_words, uint32_t *bits, int32_t *bad, hipStream_t stream);

// The label form of `who` (shape, intensity, texture, depth): the arguments that name the label maps and the windows of their labels are checked,
// then the windows are filled (the scatter step).  SDSM_OK: the entry goes on with its *_objects_impl on the windows.
static int label_windows(const char *who, const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                         const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                         int64_t window_words, uint32_t *d_bits, int32_t *d_bad, void *stream)
{
    if (n < 0 || window_words < 0 || window_words > SDSM_SHAPE_MAX_WINDOW_WORDS)
        return fail(SDSM_ERR_ARGUMENT, std::string(who) + ": n >= 0 and 0 <= window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS required");
    const char *why = !d_labels || !rec_off || !n_labels || !d_label_obj || !d_bad ? "null argument"
                                                                                    : packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits);
    if (why || !label_records_ok(n_images, n_labels, rec_off, false, &why)) return fail(SDSM_ERR_ARGUMENT, std::string(who) + ": " + why);
    hipError_t e = sdsm_shape_scatter_impl(images, n_images, d_labels, rec_off, n_labels, d_label_obj, n, d_boxes, d_bits_off, window_words, d_bits, d_bad,
                                           (hipStream_t)stream);
    SET_DONE(who);
}

extern "C" int sdsm_shape_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                        const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_slot_off, int32_t *d_slots,
                                        sdsm_shape_record *d_out, int64_t *d_vert_off, int32_t *d_verts, void *stream)
{
    SET_TABLE("sdsm_shape_objects", SET_SIDES | SET_PIXELS);
    if (const char *why = packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits))
        return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_shape_objects: ") + why);
    if (!d_vert_off || (n > 0 && (!d_slot_off || !d_slots || !d_out || !d_verts))) return fail(SDSM_ERR_ARGUMENT, "sdsm_shape_objects: null argument");
    hipError_t e = sdsm_shape_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_slot_off, d_slots, d_out, d_vert_off, d_verts,
                                           (hipStream_t)stream);
    SET_DONE("sdsm_shape_objects");
}

extern "C" int sdsm_shape_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_slot_off,
                                  int32_t *d_slots, sdsm_shape_record *d_out, int64_t *d_vert_off, int32_t *d_verts, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_shape_objects_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_slot_off, d_slots, d_out, d_vert_off, d_verts, stream);
}

extern "C" int sdsm_shape_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                                       const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                                       int64_t window_words, uint32_t *d_bits, const int64_t *d_slot_off, int32_t *d_slots, sdsm_shape_record *d_out,
                                       int64_t *d_vert_off, int32_t *d_verts, int32_t *d_bad, void *stream)
{
    SET_TABLE("sdsm_shape_labels", SET_SIDES | SET_PIXELS);
    if (!d_vert_off || (n > 0 && (!d_slot_off || !d_slots || !d_out || !d_verts))) return fail(SDSM_ERR_ARGUMENT, "sdsm_shape_labels: null argument");
    if (int rc = label_windows("sdsm_shape_labels", images, n_images, d_labels, rec_off, n_labels, d_label_obj, n, d_obj_image, d_boxes, d_bits_off, window_words,
                               d_bits, d_bad, stream))
        return rc;
    hipError_t e = sdsm_shape_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_slot_off, d_slots, d_out, d_vert_off, d_verts,
                                           (hipStream_t)stream);
    SET_DONE("sdsm_shape_labels");
}

extern "C" int sdsm_shape_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                                 const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const int64_t *d_slot_off, int32_t *d_slots,
                                 sdsm_shape_record *d_out, int64_t *d_vert_off, int32_t *d_verts, int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_shape_labels_multi(&one, 1, d_labels, &off, &n_labels, d_label_obj, n, nullptr, d_boxes, d_bits_off, window_words, d_bits, d_slot_off, d_slots,
                                   d_out, d_vert_off, d_verts, d_bad, stream);
}

// ---- intensity distribution tables (sdsm_intensity.hip; the label form fills its windows with the scatter step of sdsm_shape.hip) -------
extern "C" hipError_t sdsm_intensity_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                  const int64_t *bits_off, const uint32_t *bits, const double *d_g, int n_q, const int32_t *num,
                                                  const int32_t *den, sdsm_intensity_record *out, double *order, hipStream_t stream);

static bool quantiles_ok(int n_q, const int32_t *num, const int32_t *den)
{
    if (n_q < 0 || n_q > SDSM_INTENSITY_MAX_QUANTILES || (n_q > 0 && (!num || !den))) return false;
    for (int q = 0; q < n_q; q++)
        if (den[q] < 1 || den[q] > SDSM_INTENSITY_MAX_DEN || num[q] < 0 || num[q] > den[q]) return false;
    return true;
}

extern "C" int sdsm_intensity_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                            const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, int n_q, const int32_t *num,
                                            const int32_t *den, sdsm_intensity_record *d_out, double *d_order, void *stream)
{
    SET_TABLE("sdsm_intensity_objects", SET_SIDES | SET_PIXELS);
    if (const char *why = packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits))
        return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_intensity_objects: ") + why);
    if (!quantiles_ok(n_q, num, den))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_intensity_objects: 0 <= n_q <= 8 quantiles with 0 <= num <= den, 1 <= den <= 1000000 required");
    if (n > 0 && (!d_g || !d_out || (n_q > 0 && !d_order))) return fail(SDSM_ERR_ARGUMENT, "sdsm_intensity_objects: null argument");
    hipError_t e = sdsm_intensity_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, n_q, num, den, d_out, d_order,
                                               (hipStream_t)stream);
    SET_DONE("sdsm_intensity_objects");
}

extern "C" int sdsm_intensity_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                                      int n_q, const int32_t *num, const int32_t *den, sdsm_intensity_record *d_out, double *d_order, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_intensity_objects_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_g, n_q, num, den, d_out, d_order, stream);
}

extern "C" int sdsm_intensity_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off,
                                           const int32_t *n_labels, const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                           const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int n_q,
                                           const int32_t *num, const int32_t *den, sdsm_intensity_record *d_out, double *d_order, int32_t *d_bad,
                                           void *stream)
{
    SET_TABLE("sdsm_intensity_labels", SET_SIDES | SET_PIXELS);
    if (!quantiles_ok(n_q, num, den))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_intensity_labels: 0 <= n_q <= 8 quantiles with 0 <= num <= den, 1 <= den <= 1000000 required");
    if (n > 0 && (!d_g || !d_out || (n_q > 0 && !d_order))) return fail(SDSM_ERR_ARGUMENT, "sdsm_intensity_labels: null argument");
    if (int rc = label_windows("sdsm_intensity_labels", images, n_images, d_labels, rec_off, n_labels, d_label_obj, n, d_obj_image, d_boxes, d_bits_off,
                               window_words, d_bits, d_bad, stream))
        return rc;
    hipError_t e = sdsm_intensity_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, n_q, num, den, d_out, d_order,
                                               (hipStream_t)stream);
    SET_DONE("sdsm_intensity_labels");
}

extern "C" int sdsm_intensity_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                                     const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int n_q, const int32_t *num,
                                     const int32_t *den, sdsm_intensity_record *d_out, double *d_order, int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_intensity_labels_multi(&one, 1, d_labels, &off, &n_labels, d_label_obj, n, nullptr, d_boxes, d_bits_off, window_words, d_bits, d_g, n_q,
                                       num, den, d_out, d_order, d_bad, stream);
}

// ---- texture tables (sdsm_texture.hip; the label form fills its windows with the scatter step of sdsm_shape.hip) -----------------------
extern "C" hipError_t sdsm_texture_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                const int64_t *bits_off, const uint32_t *bits, const double *d_g, int levels, const double *d_edges,
                                                int n_offsets, const int32_t *offsets, const int64_t *slot_off, sdsm_texture_entry *slots,
                                                sdsm_texture_record *out, sdsm_texture_pairs *pairs, sdsm_texture_entry *entries, hipStream_t stream);

// the offsets of a call: 1 .. 8 pairs, none (0, 0), reach <= 32, none twice or together with its negative
static bool texture_offsets_ok(int n_offsets, const int32_t *offsets)
{
    if (n_offsets < 1 || n_offsets > SDSM_TEXTURE_MAX_OFFSETS || !offsets) return false;
    for (int o = 0; o < n_offsets; o++) {
        const int dr = offsets[2 * o], dc = offsets[2 * o + 1];
        if ((dr == 0 && dc == 0) || dr < -SDSM_TEXTURE_MAX_REACH || dr > SDSM_TEXTURE_MAX_REACH || dc < -SDSM_TEXTURE_MAX_REACH || dc > SDSM_TEXTURE_MAX_REACH)
            return false;
        for (int p = 0; p < o; p++)
            if ((offsets[2 * p] == dr && offsets[2 * p + 1] == dc) || (offsets[2 * p] == -dr && offsets[2 * p + 1] == -dc)) return false;
    }
    return true;
}

#define TEXTURE_ARGS(name) \
    if (n < 0 || n > INT_MAX / SDSM_TEXTURE_MAX_OFFSETS) return fail(SDSM_ERR_ARGUMENT, name ": 0 <= n <= (2^31 - 1) / 8 required"); \
    if (levels < 1 || levels > SDSM_TEXTURE_MAX_LEVELS) return fail(SDSM_ERR_ARGUMENT, name ": 1 <= levels <= 256 required"); \
    if (!texture_offsets_ok(n_offsets, offsets)) \
        return fail(SDSM_ERR_ARGUMENT, name ": 1 <= n_offsets <= 8 offsets, none (0, 0), |d_row|, |d_col| <= 32, none twice or with its negative required"); \
    if (n > 0 && (!d_g || (levels > 1 && !d_edges) || !d_slot_off || !d_slots || !d_out || !d_pairs || !d_entries)) \
        return fail(SDSM_ERR_ARGUMENT, name ": null argument")

extern "C" int sdsm_texture_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                          const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, int levels, const double *d_edges,
                                          int n_offsets, const int32_t *offsets, const int64_t *d_slot_off, sdsm_texture_entry *d_slots,
                                          sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs, sdsm_texture_entry *d_entries, void *stream)
{
    SET_TABLE("sdsm_texture_objects", SET_SIDES | SET_PIXELS);
    TEXTURE_ARGS("sdsm_texture_objects");
    if (const char *why = packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits))
        return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_texture_objects: ") + why);
    hipError_t e = sdsm_texture_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, levels, d_edges, n_offsets, offsets,
                                             d_slot_off, d_slots, d_out, d_pairs, d_entries, (hipStream_t)stream);
    SET_DONE("sdsm_texture_objects");
}

extern "C" int sdsm_texture_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                                    int levels, const double *d_edges, int n_offsets, const int32_t *offsets, const int64_t *d_slot_off,
                                    sdsm_texture_entry *d_slots, sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs, sdsm_texture_entry *d_entries,
                                    void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_texture_objects_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_g, levels, d_edges, n_offsets, offsets, d_slot_off, d_slots, d_out,
                                      d_pairs, d_entries, stream);
}

extern "C" int sdsm_texture_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off,
                                         const int32_t *n_labels, const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                         const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int levels,
                                         const double *d_edges, int n_offsets, const int32_t *offsets, const int64_t *d_slot_off,
                                         sdsm_texture_entry *d_slots, sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs,
                                         sdsm_texture_entry *d_entries, int32_t *d_bad, void *stream)
{
    SET_TABLE("sdsm_texture_labels", SET_SIDES | SET_PIXELS);
    TEXTURE_ARGS("sdsm_texture_labels");
    if (window_words < 0 || window_words > SDSM_SHAPE_MAX_WINDOW_WORDS)      // (n is checked above: this entry's text names the words alone)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_texture_labels: 0 <= window_words <= SDSM_SHAPE_MAX_WINDOW_WORDS required");
    if (int rc = label_windows("sdsm_texture_labels", images, n_images, d_labels, rec_off, n_labels, d_label_obj, n, d_obj_image, d_boxes, d_bits_off,
                               window_words, d_bits, d_bad, stream))
        return rc;
    hipError_t e = sdsm_texture_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, levels, d_edges, n_offsets, offsets, d_slot_off,
                                             d_slots, d_out, d_pairs, d_entries, (hipStream_t)stream);
    SET_DONE("sdsm_texture_labels");
}

extern "C" int sdsm_texture_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                                   const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, int levels,
                                   const double *d_edges, int n_offsets, const int32_t *offsets, const int64_t *d_slot_off, sdsm_texture_entry *d_slots,
                                   sdsm_texture_record *d_out, sdsm_texture_pairs *d_pairs, sdsm_texture_entry *d_entries, int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_texture_labels_multi(&one, 1, d_labels, &off, &n_labels, d_label_obj, n, nullptr, d_boxes, d_bits_off, window_words, d_bits, d_g, levels,
                                     d_edges, n_offsets, offsets, d_slot_off, d_slots, d_out, d_pairs, d_entries, d_bad, stream);
}

// ---- depth tables (sdsm_depth.hip; the scale step of sdsm_measure.hip, the label form fills its windows with the scatter step of
// sdsm_shape.hip) ---------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t sdsm_measure_scale_impl(const sdsm_set_image *images, int n_images, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                              hipStream_t stream);
extern "C" hipError_t sdsm_depth_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                              const int64_t *bits_off, const uint32_t *bits, const double *d_g, const double *d_gmax_abs, int n_shells,
                                              const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, sdsm_depth_record *out,
                                              sdsm_depth_shell_record *shells, hipStream_t stream);

// the shells, the intensity buffers, the workspace and the outputs of a call for n objects; null: fine
static const char *depth_args_bad(int n, int n_shells, const double *d_g, const double *d_gmax_abs, const int64_t *d_ws_off, const void *d_ws, int64_t ws_pixels,
                                  size_t ws_bytes, const void *d_out, const void *d_shells)
{
    if (n_shells < 1 || n_shells > SDSM_DEPTH_MAX_SHELLS) return "1 <= n_shells <= 32 required";
    if (d_g && !d_gmax_abs) return "intensities need d_gmax_abs";
    if (ws_pixels < 0 || (ws_pixels > 0 && (!d_ws_off || !d_ws))) return "ws_pixels >= 0 and, with ws_pixels > 0, d_ws_off and d_ws required";
    if ((uint64_t)ws_pixels > ws_bytes / SDSM_DEPTH_WS_PIXEL_BYTES) return "the workspace is too small for the boxes named (8 bytes per pixel)";
    if (n > 0 && (!d_out || !d_shells)) return "null argument";
    return nullptr;
}

extern "C" int sdsm_depth_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                        const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                        int n_shells, const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, size_t ws_bytes, sdsm_depth_record *d_out,
                                        sdsm_depth_shell_record *d_shells, void *stream)
{
    SET_TABLE("sdsm_depth_objects", SET_SIDES | SET_PIXELS);
    const char *why = packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits);
    if (!why) why = depth_args_bad(n, n_shells, d_g, d_gmax_abs, d_ws_off, d_ws, ws_pixels, ws_bytes, d_out, d_shells);
    if (why) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_depth_objects: ") + why);
    hipError_t e = sdsm_measure_scale_impl(images, n_images, d_g, d_gmax_abs, d_scale_exp, (hipStream_t)stream);
    if (e == hipSuccess)
        e = sdsm_depth_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, d_gmax_abs, n_shells, d_ws_off, d_ws, ws_pixels, d_out,
                                    d_shells, (hipStream_t)stream);
    SET_DONE("sdsm_depth_objects");
}

extern "C" int sdsm_depth_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g,
                                  double *d_gmax_abs, int32_t *d_scale_exp, int n_shells, const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels,
                                  size_t ws_bytes, sdsm_depth_record *d_out, sdsm_depth_shell_record *d_shells, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_depth_objects_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_g, d_gmax_abs, d_scale_exp, n_shells, d_ws_off, d_ws, ws_pixels,
                                    ws_bytes, d_out, d_shells, stream);
}

extern "C" int sdsm_depth_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                                       const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                                       int64_t window_words, uint32_t *d_bits, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp, int n_shells,
                                       const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, size_t ws_bytes, sdsm_depth_record *d_out,
                                       sdsm_depth_shell_record *d_shells, int32_t *d_bad, void *stream)
{
    SET_TABLE("sdsm_depth_labels", SET_SIDES | SET_PIXELS);
    if (const char *why = depth_args_bad(n, n_shells, d_g, d_gmax_abs, d_ws_off, d_ws, ws_pixels, ws_bytes, d_out, d_shells))
        return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_depth_labels: ") + why);
    if (int rc = label_windows("sdsm_depth_labels", images, n_images, d_labels, rec_off, n_labels, d_label_obj, n, d_obj_image, d_boxes, d_bits_off, window_words,
                               d_bits, d_bad, stream))
        return rc;
    hipError_t e = sdsm_measure_scale_impl(images, n_images, d_g, d_gmax_abs, d_scale_exp, (hipStream_t)stream);
    if (e == hipSuccess)
        e = sdsm_depth_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_g, d_gmax_abs, n_shells, d_ws_off, d_ws, ws_pixels, d_out,
                                    d_shells, (hipStream_t)stream);
    SET_DONE("sdsm_depth_labels");
}

extern "C" int sdsm_depth_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                                 const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const double *d_g, double *d_gmax_abs,
                                 int32_t *d_scale_exp, int n_shells, const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, size_t ws_bytes,
                                 sdsm_depth_record *d_out, sdsm_depth_shell_record *d_shells, int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_depth_labels_multi(&one, 1, d_labels, &off, &n_labels, d_label_obj, n, nullptr, d_boxes, d_bits_off, window_words, d_bits, d_g, d_gmax_abs,
                                   d_scale_exp, n_shells, d_ws_off, d_ws, ws_pixels, ws_bytes, d_out, d_shells, d_bad, stream);
}

// ---- skeleton tables (sdsm_skeleton.hip; the label form fills its windows with the scatter step of sdsm_shape.hip) --------------------------
extern "C" hipError_t sdsm_skeleton_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                 const int64_t *bits_off, const uint32_t *bits, const int64_t *d_ws_off, void *d_ws, int64_t ws_words,
                                                 sdsm_skeleton_record *out, uint32_t *skel, const int32_t *obj_label, int32_t *map, hipStream_t stream);

// the workspace and the outputs of a call for n objects; null: fine
static const char *skeleton_args_bad(int n, const int64_t *d_ws_off, const void *d_ws, int64_t ws_words, size_t ws_bytes, const void *d_out, const void *d_skeleton)
{
    if (ws_words < 0 || (ws_words > 0 && (!d_ws_off || !d_ws))) return "ws_words >= 0 and, with ws_words > 0, d_ws_off and d_ws required";
    if ((uint64_t)ws_words > ws_bytes / 8) return "the workspace is too small for the boxes named (8 bytes per word)";
    if (n > 0 && (!d_out || !d_skeleton)) return "null argument";
    return nullptr;
}

extern "C" int sdsm_skeleton_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                           const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_ws_off, void *d_ws, int64_t ws_words,
                                           size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, void *stream)
{
    SET_TABLE("sdsm_skeleton_objects", SET_SIDES | SET_PIXELS);
    const char *why = packed_objects_bad(n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits);
    if (!why) why = skeleton_args_bad(n, d_ws_off, d_ws, ws_words, ws_bytes, d_out, d_skeleton);
    if (why) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_skeleton_objects: ") + why);
    hipError_t e = sdsm_skeleton_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_ws_off, d_ws, ws_words, d_out, d_skeleton, nullptr,
                                              nullptr, (hipStream_t)stream);
    SET_DONE("sdsm_skeleton_objects");
}

extern "C" int sdsm_skeleton_objects(int H, int W, int n, const int32_t *d_boxes, const int64_t *d_bits_off, const uint32_t *d_bits, const int64_t *d_ws_off,
                                     void *d_ws, int64_t ws_words, size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_skeleton_objects_multi(&one, 1, n, nullptr, d_boxes, d_bits_off, d_bits, d_ws_off, d_ws, ws_words, ws_bytes, d_out, d_skeleton, stream);
}

extern "C" int sdsm_skeleton_labels_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int64_t *rec_off, const int32_t *n_labels,
                                          const int32_t *d_label_obj, int n, const int32_t *d_obj_image, const int32_t *d_boxes, const int64_t *d_bits_off,
                                          int64_t window_words, uint32_t *d_bits, const int32_t *d_obj_label, const int64_t *d_ws_off, void *d_ws,
                                          int64_t ws_words, size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, int32_t *d_map, int32_t *d_bad,
                                          void *stream)
{
    SET_TABLE("sdsm_skeleton_labels", SET_SIDES | SET_PIXELS);
    const char *why = skeleton_args_bad(n, d_ws_off, d_ws, ws_words, ws_bytes, d_out, d_skeleton);
    if (!why && n > 0 && !d_obj_label) why = "null argument";
    if (why) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_skeleton_labels: ") + why);
    if (int rc = label_windows("sdsm_skeleton_labels", images, n_images, d_labels, rec_off, n_labels, d_label_obj, n, d_obj_image, d_boxes, d_bits_off,
                               window_words, d_bits, d_bad, stream))
        return rc;
    hipError_t e = hipSuccess;
    for (int i = 0; d_map && i < n_images && e == hipSuccess; i++)
        e = hipMemsetAsync(d_map + images[i].offset, 0, sizeof(int32_t) * (size_t)images[i].H * (size_t)images[i].W, (hipStream_t)stream);
    if (e == hipSuccess)
        e = sdsm_skeleton_objects_impl(images, n_images, n, d_obj_image, d_boxes, d_bits_off, d_bits, d_ws_off, d_ws, ws_words, d_out, d_skeleton, d_obj_label,
                                       d_map, (hipStream_t)stream);
    SET_DONE("sdsm_skeleton_labels");
}

extern "C" int sdsm_skeleton_labels(int H, int W, const int32_t *d_labels, int n_labels, const int32_t *d_label_obj, int n, const int32_t *d_boxes,
                                    const int64_t *d_bits_off, int64_t window_words, uint32_t *d_bits, const int32_t *d_obj_label, const int64_t *d_ws_off,
                                    void *d_ws, int64_t ws_words, size_t ws_bytes, sdsm_skeleton_record *d_out, uint32_t *d_skeleton, int32_t *d_map,
                                    int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_skeleton_labels_multi(&one, 1, d_labels, &off, &n_labels, d_label_obj, n, nullptr, d_boxes, d_bits_off, window_words, d_bits, d_obj_label,
                                      d_ws_off, d_ws, ws_words, ws_bytes, d_out, d_skeleton, d_map, d_bad, stream);
}

// ---- contingency table of two label maps (sdsm_measure.hip) ---------------------------------------------------------------------------
extern "C" hipError_t sdsm_overlap_pairs_impl(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b,
                                              const int64_t *table_off, const int64_t *capacity, uint64_t *d_keys, uint64_t *d_counts,
                                              int32_t *d_status, hipStream_t stream);

extern "C" int sdsm_overlap_pairs_multi(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b, const int64_t *table_off,
                                        const int64_t *capacity, uint64_t *d_keys, uint64_t *d_counts, int32_t *d_status, void *stream)
{
    SET_TABLE("sdsm_overlap_pairs", SET_PIXELS);
    if (!d_a || !d_b || !table_off || !capacity || !d_keys || !d_counts || !d_status) return fail(SDSM_ERR_ARGUMENT, "sdsm_overlap_pairs: null argument");
    const char *why;
    if (!pair_tables_ok(n_images, table_off, capacity, &why)) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_overlap_pairs: ") + why);
    hipError_t e = sdsm_overlap_pairs_impl(images, n_images, d_a, d_b, table_off, capacity, d_keys, d_counts, d_status, (hipStream_t)stream);
    SET_DONE("sdsm_overlap_pairs");
}

extern "C" int sdsm_overlap_pairs(int H, int W, const int32_t *d_a, const int32_t *d_b, int64_t capacity, uint64_t *d_keys, uint64_t *d_counts,
                                  int32_t *d_status, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_overlap_pairs_multi(&one, 1, d_a, d_b, &off, &capacity, d_keys, d_counts, d_status, stream);
}

// ---- neighbourhood tables of one label map (sdsm_neighbours.hip) -----------------------------------------------------------------------
extern "C" hipError_t sdsm_neighbours_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, const int64_t *rec_off,
                                           const int32_t *n_labels, sdsm_neighbour_label *d_label_out, const int64_t *table_off,
                                           const int64_t *capacity, uint64_t *d_keys, uint32_t *d_min_d2, uint32_t *d_contact, int32_t *d_status,
                                           hipStream_t stream);

extern "C" int sdsm_neighbours_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, const int64_t *rec_off,
                                     const int32_t *n_labels, sdsm_neighbour_label *d_label_out, const int64_t *table_off, const int64_t *capacity,
                                     uint64_t *d_keys, uint32_t *d_min_d2, uint32_t *d_contact, int32_t *d_status, void *stream)
{
    if (max_d2 < 1 || max_d2 > SDSM_NEIGHBOUR_MAX_D2) return fail(SDSM_ERR_ARGUMENT, "sdsm_neighbours: 1 <= max_d2 <= 4096 required");
    SET_TABLE("sdsm_neighbours", 0);
    if (!boundary_shapes_ok(images, n_images)) return fail(SDSM_ERR_ARGUMENT, "sdsm_neighbours: H * H + W * W < 2^31 required");
    if (!d_labels || !rec_off || !n_labels || !d_label_out || !table_off || !capacity || !d_keys || !d_min_d2 || !d_contact || !d_status)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_neighbours: null argument");
    const char *why_l, *why_t;                   // both walks; what the walk over the images meets first is reported (labels before tables)
    int at_l, at_t;
    const bool l_ok = label_records_ok(n_images, n_labels, rec_off, true, &why_l, &at_l), t_ok = pair_tables_ok(n_images, table_off, capacity, &why_t, &at_t);
    if (!l_ok || !t_ok) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_neighbours: ") + (!l_ok && (t_ok || at_l <= at_t) ? why_l : why_t));
    hipError_t e = sdsm_neighbours_impl(images, n_images, d_labels, max_d2, rec_off, n_labels, d_label_out, table_off, capacity, d_keys, d_min_d2,
                                        d_contact, d_status, (hipStream_t)stream);
    SET_DONE("sdsm_neighbours");
}

extern "C" int sdsm_neighbours(int H, int W, const int32_t *d_labels, int max_d2, int n_labels, sdsm_neighbour_label *d_label_out, int64_t capacity,
                               uint64_t *d_keys, uint32_t *d_min_d2, uint32_t *d_contact, int32_t *d_status, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_neighbours_multi(&one, 1, d_labels, max_d2, &off, &n_labels, d_label_out, &off, &capacity, d_keys, d_min_d2, d_contact, d_status, stream);
}

// ---- zone label maps of one label map (sdsm_zones.hip) -----------------------------------------------------------------------------------
extern "C" hipError_t sdsm_zones_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, int n_zones,
                                      const sdsm_zone_spec *zones, int64_t zone_stride, int32_t *d_d2, int32_t *d_other, int32_t *d_zone_out,
                                      int32_t *d_status, hipStream_t stream);

// a bound of a zone: 0 .. max_d2
static bool zone_bound_ok(int32_t v, int max_d2) { return v >= 0 && v <= max_d2; }

extern "C" int sdsm_zones_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, int n_zones, const sdsm_zone_spec *zones,
                                int64_t zone_stride, int32_t *d_d2, int32_t *d_other, int32_t *d_zone_out, int32_t *d_status, void *stream)
{
    if (max_d2 < 1 || max_d2 > SDSM_ZONE_MAX_D2) return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: 1 <= max_d2 <= 4096 required");
    if (n_zones < 0 || n_zones > SDSM_ZONE_MAX_ZONES) return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: 0 <= n_zones <= 8 required");
    SET_TABLE("sdsm_zones", 0);
    if (!boundary_shapes_ok(images, n_images)) return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: H * H + W * W < 2^31 required");
    if (!d_labels || !d_status || (n_zones > 0 && (!zones || !d_zone_out))) return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: null argument");
    for (int z = 0; z < n_zones; z++) {
        const sdsm_zone_spec &Z = zones[z];
        const bool object = Z.side == SDSM_ZONE_SIDE_OBJECT;
        if ((!object && Z.side != SDSM_ZONE_SIDE_BACKGROUND) || (Z.keep_own != 0 && (Z.keep_own != 1 || object)))
            return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: a zone's side is 0 or 1, keep_own 0 or, on the background side, 1");
        if (!zone_bound_ok(Z.lo_d2, max_d2) || !(zone_bound_ok(Z.hi_d2, max_d2) || (object && Z.hi_d2 == SDSM_ZONE_NO_UPPER)) || Z.lo_d2 >= Z.hi_d2)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: 0 <= lo_d2 < hi_d2 <= max_d2 required (hi_d2 of an object zone may be SDSM_ZONE_NO_UPPER)");
    }
    for (int i = 0; n_zones > 0 && i < n_images; i++)
        if (zone_stride < images[i].offset + (int64_t)images[i].H * images[i].W)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_zones: zone_stride >= offset + H * W of every image required");
    hipError_t e = sdsm_zones_impl(images, n_images, d_labels, max_d2, n_zones, zones, zone_stride, d_d2, d_other, d_zone_out, d_status, (hipStream_t)stream);
    SET_DONE("sdsm_zones");
}

extern "C" int sdsm_zones(int H, int W, const int32_t *d_labels, int max_d2, int n_zones, const sdsm_zone_spec *zones, int32_t *d_d2, int32_t *d_other,
                          int32_t *d_zone_out, int32_t *d_status, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_zones_multi(&one, 1, d_labels, max_d2, n_zones, zones, (int64_t)H * W, d_d2, d_other, d_zone_out, d_status, stream);
}

// ---- connected parts of one label map (sdsm_parts.hip) -----------------------------------------------------------------------------------
extern "C" size_t sdsm_parts_workspace_bytes_impl(const sdsm_set_image *images, int n_images, const int64_t *rec_off, const int32_t *n_labels);
extern "C" hipError_t sdsm_parts_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int connectivity, const int64_t *rec_off,
                                      const int32_t *n_labels, sdsm_part_label_record *d_label_out, int32_t *d_part_map, int32_t *d_count,
                                      int32_t *d_status, void *d_ws, hipStream_t stream);
extern "C" hipError_t sdsm_parts_table_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map,
                                            const int64_t *part_off, const int32_t *n_parts, sdsm_part_record *d_part_out, hipStream_t stream);
extern "C" hipError_t sdsm_parts_keep_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map,
                                           const int64_t *rec_off, const int32_t *n_labels, const sdsm_part_label_record *d_label_recs,
                                           const int64_t *part_off, const int32_t *n_parts, const sdsm_part_record *d_part_recs, int n_keeps,
                                           const sdsm_keep_spec *keeps, int64_t keep_stride, int32_t *d_keep_out, hipStream_t stream);

// the part records of a set: n_parts[i] >= 0 records from part_off[i] on
static bool part_records_ok(int n_images, const int32_t *n_parts, const int64_t *part_off, bool check_overlap, const char **why)
{
    return ranges_ok(n_images, part_off, n_parts, [](int32_t n) { return n >= 0; }, check_overlap, "n_parts >= 0 and part_off >= 0 required",
                     "the part records of two images overlap", why, nullptr);
}

extern "C" size_t sdsm_parts_workspace_bytes_multi(const sdsm_set_image *images, int n_images, const int64_t *rec_off, const int32_t *n_labels)
{
    const char *why;
    if (!set_table_ok(images, n_images, 0) || !boundary_shapes_ok(images, n_images) || !rec_off || !n_labels) return 0;
    return label_records_ok(n_images, n_labels, rec_off, true, &why) ? sdsm_parts_workspace_bytes_impl(images, n_images, rec_off, n_labels) : 0;
}

extern "C" int sdsm_parts_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int connectivity, const int64_t *rec_off,
                                const int32_t *n_labels, sdsm_part_label_record *d_label_out, int32_t *d_part_map, int32_t *d_count, int32_t *d_status,
                                void *d_ws, size_t ws_bytes, void *stream)
{
    if (connectivity != 4 && connectivity != 8) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts: connectivity 4 or 8 required");
    SET_TABLE("sdsm_parts", 0);
    if (!boundary_shapes_ok(images, n_images)) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts: H * H + W * W < 2^31 required");
    if (!d_labels || !rec_off || !n_labels || !d_label_out || !d_part_map || !d_count || !d_status || !d_ws)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_parts: null argument");
    const char *why;
    if (!label_records_ok(n_images, n_labels, rec_off, true, &why)) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_parts: ") + why);
    if (((uintptr_t)d_ws & 7) != 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts: the workspace must be 8-byte aligned");
    if (ws_bytes < sdsm_parts_workspace_bytes_impl(images, n_images, rec_off, n_labels)) return fail(SDSM_ERR_WORKSPACE, "sdsm_parts: workspace too small");
    hipError_t e = sdsm_parts_impl(images, n_images, d_labels, connectivity, rec_off, n_labels, d_label_out, d_part_map, d_count, d_status, d_ws,
                                   (hipStream_t)stream);
    SET_DONE("sdsm_parts");
}

extern "C" int sdsm_parts(int H, int W, const int32_t *d_labels, int connectivity, int n_labels, sdsm_part_label_record *d_label_out, int32_t *d_part_map,
                          int32_t *d_count, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    const int64_t off = 0;
    return sdsm_parts_multi(&one, 1, d_labels, connectivity, &off, &n_labels, d_label_out, d_part_map, d_count, d_status, d_ws, ws_bytes, stream);
}

extern "C" int sdsm_parts_table_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map, const int64_t *part_off,
                                      const int32_t *n_parts, sdsm_part_record *d_part_out, void *stream)
{
    SET_TABLE("sdsm_parts_table", 0);
    if (!boundary_shapes_ok(images, n_images)) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_table: H * H + W * W < 2^31 required");
    if (!d_labels || !d_part_map || !part_off || !n_parts || !d_part_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_table: null argument");
    const char *why;
    if (!part_records_ok(n_images, n_parts, part_off, true, &why)) return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_parts_table: ") + why);
    hipError_t e = sdsm_parts_table_impl(images, n_images, d_labels, d_part_map, part_off, n_parts, d_part_out, (hipStream_t)stream);
    SET_DONE("sdsm_parts_table");
}

extern "C" int sdsm_parts_keep_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map, const int64_t *rec_off,
                                     const int32_t *n_labels, const sdsm_part_label_record *d_label_recs, const int64_t *part_off, const int32_t *n_parts,
                                     const sdsm_part_record *d_part_recs, int n_keeps, const sdsm_keep_spec *keeps, int64_t keep_stride, int32_t *d_keep_out,
                                     void *stream)
{
    if (n_keeps < 1 || n_keeps > SDSM_PARTS_MAX_KEEPS) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_keep: 1 <= n_keeps <= 8 required");
    SET_TABLE("sdsm_parts_keep", 0);
    if (!boundary_shapes_ok(images, n_images)) return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_keep: H * H + W * W < 2^31 required");
    if (!d_labels || !d_part_map || !rec_off || !n_labels || !d_label_recs || !part_off || !n_parts || !d_part_recs || !keeps || !d_keep_out)
        return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_keep: null argument");
    const char *why;
    if (!label_records_ok(n_images, n_labels, rec_off, false, &why) || !part_records_ok(n_images, n_parts, part_off, false, &why))
        return fail(SDSM_ERR_ARGUMENT, std::string("sdsm_parts_keep: ") + why);
    for (int z = 0; z < n_keeps; z++) {
        const sdsm_keep_spec &K = keeps[z];
        if (K.kind != SDSM_KEEP_SPLIT && K.kind != SDSM_KEEP_LARGEST && K.kind != SDSM_KEEP_MIN_AREA)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_keep: a selection's kind is 0, 1 or 2");
        if (K.kind == SDSM_KEEP_MIN_AREA ? K.min_area < 1 : K.min_area != 0)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_keep: min_area >= 1 for SDSM_KEEP_MIN_AREA, 0 for the other kinds");
    }
    for (int i = 0; i < n_images; i++)
        if (keep_stride < images[i].offset + (int64_t)images[i].H * images[i].W)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_parts_keep: keep_stride >= offset + H * W of every image required");
    hipError_t e = sdsm_parts_keep_impl(images, n_images, d_labels, d_part_map, rec_off, n_labels, d_label_recs, part_off, n_parts, d_part_recs, n_keeps, keeps,
                                        keep_stride, d_keep_out, (hipStream_t)stream);
    SET_DONE("sdsm_parts_keep");
}

// ---- boundary distances between two label maps (sdsm_measure.hip) ---------------------------------------------------------------------
extern "C" hipError_t sdsm_label_pixel_counts_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, int32_t *counts, int32_t *bad,
                                                   hipStream_t stream);
extern "C" hipError_t sdsm_label_pixel_lists_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int32_t *counts,
                                                  int32_t *start, int32_t *cursor, uint32_t *list, hipStream_t stream);
extern "C" hipError_t sdsm_pair_distances_impl(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b,
                                               const int32_t *counts_a, const int32_t *counts_b, const int32_t *start_a, const int32_t *start_b,
                                               const uint32_t *list_a, const uint32_t *list_b, int n_pairs, const int32_t *pairs, int64_t n_items,
                                               const int32_t *items, sdsm_pair_distance *recs, hipStream_t stream);
extern "C" void sdsm_quantised_distance_impl(const int32_t *d2, int64_t n, int64_t *out);

#define BOUNDARY_TABLE(name) \
    SET_TABLE(name, 0); \
    if (!boundary_shapes_ok(images, n_images)) return fail(SDSM_ERR_ARGUMENT, name ": H * H + W * W < 2^31 required")

extern "C" int sdsm_label_pixel_counts_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int32_t *d_counts, int32_t *d_bad,
                                             void *stream)
{
    BOUNDARY_TABLE("sdsm_label_pixel_counts");
    if (!d_labels || !d_counts || !d_bad) return fail(SDSM_ERR_ARGUMENT, "sdsm_label_pixel_counts: null argument");
    hipError_t e = sdsm_label_pixel_counts_impl(images, n_images, d_labels, d_counts, d_bad, (hipStream_t)stream);
    SET_DONE("sdsm_label_pixel_counts");
}

extern "C" int sdsm_label_pixel_counts(int H, int W, const int32_t *d_labels, int32_t *d_counts, int32_t *d_bad, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_label_pixel_counts_multi(&one, 1, d_labels, d_counts, d_bad, stream);
}

extern "C" int sdsm_label_pixel_lists_multi(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_counts,
                                            int32_t *d_start, int32_t *d_cursor, uint32_t *d_list, void *stream)
{
    BOUNDARY_TABLE("sdsm_label_pixel_lists");
    if (!d_labels || !d_counts || !d_start || !d_cursor || !d_list) return fail(SDSM_ERR_ARGUMENT, "sdsm_label_pixel_lists: null argument");
    hipError_t e = sdsm_label_pixel_lists_impl(images, n_images, d_labels, d_counts, d_start, d_cursor, d_list, (hipStream_t)stream);
    SET_DONE("sdsm_label_pixel_lists");
}

extern "C" int sdsm_label_pixel_lists(int H, int W, const int32_t *d_labels, const int32_t *d_counts, int32_t *d_start, int32_t *d_cursor,
                                      uint32_t *d_list, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_label_pixel_lists_multi(&one, 1, d_labels, d_counts, d_start, d_cursor, d_list, stream);
}

extern "C" int sdsm_pair_distances_multi(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b, const int32_t *d_counts_a,
                                         const int32_t *d_counts_b, const int32_t *d_start_a, const int32_t *d_start_b, const uint32_t *d_list_a,
                                         const uint32_t *d_list_b, int n_pairs, const int32_t *d_pairs, int64_t n_items, const int32_t *d_items,
                                         sdsm_pair_distance *d_records, void *stream)
{
    BOUNDARY_TABLE("sdsm_pair_distances");
    if (n_pairs < 0 || n_items < 0 || n_items > INT_MAX) return fail(SDSM_ERR_ARGUMENT, "sdsm_pair_distances: 0 <= n_pairs, 0 <= n_items < 2^31 required");
    if (n_pairs == 0) return SDSM_OK;
    if (!d_a || !d_b || !d_counts_a || !d_counts_b || !d_start_a || !d_start_b || !d_list_a || !d_list_b || !d_pairs || !d_records || (n_items > 0 && !d_items))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_pair_distances: null argument");
    hipError_t e = sdsm_pair_distances_impl(images, n_images, d_a, d_b, d_counts_a, d_counts_b, d_start_a, d_start_b, d_list_a, d_list_b, n_pairs, d_pairs,
                                            n_items, d_items, d_records, (hipStream_t)stream);
    SET_DONE("sdsm_pair_distances");
}

extern "C" int sdsm_pair_distances(int H, int W, const int32_t *d_a, const int32_t *d_b, const int32_t *d_counts_a, const int32_t *d_counts_b,
                                   const int32_t *d_start_a, const int32_t *d_start_b, const uint32_t *d_list_a, const uint32_t *d_list_b, int n_pairs,
                                   const int32_t *d_pairs, int64_t n_items, const int32_t *d_items, sdsm_pair_distance *d_records, void *stream)
{
    const sdsm_set_image one = {0, H, W};
    return sdsm_pair_distances_multi(&one, 1, d_a, d_b, d_counts_a, d_counts_b, d_start_a, d_start_b, d_list_a, d_list_b, n_pairs, d_pairs, n_items, d_items,
                                     d_records, stream);
}

extern "C" int sdsm_quantised_distance(const int32_t *d2, int64_t n, int64_t *out)
{
    if (n < 0 || (n > 0 && (!d2 || !out))) return fail(SDSM_ERR_ARGUMENT, "sdsm_quantised_distance: null argument");
    sdsm_quantised_distance_impl(d2, n, out);
    return SDSM_OK;
}

extern "C" int sdsm_post_background_multi(const sdsm_post_bg_image *images, int n_images, const int32_t *d_boxes, const int64_t *d_bits_off,
                                          const uint32_t *d_bits, int radius, void *stream)
{
    SET_TABLE("sdsm_post_background_multi", SET_SIDES | SET_PIXELS);
    if (radius < 0 || radius > SDSM_POST_MAX_BG_RADIUS) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_background_multi: 0 <= radius <= 32 required");
    int64_t n = 0, tiles = 0;
    for (int j = 0; j < n_images; j++) {
        const sdsm_post_bg_image &im = images[j];
        if (im.n_objects < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_background_multi: negative object count");
        if (!im.d_bg || !im.d_work) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_background_multi: null image buffer");
        n += im.n_objects;
        tiles += ((int64_t)im.H * im.W + 255) / 256;
    }
    if (n >= (1 << 30) || tiles >= INT_MAX) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_background_multi: more than 2^30 - 1 objects or 2^39 pixels");
    if (n > 0 && (!d_boxes || !d_bits_off || !d_bits)) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_background_multi: null argument");
    hipError_t e = sdsm_launch_post_background(images, n_images, d_boxes, d_bits_off, d_bits, radius, (hipStream_t)stream);
    SET_DONE("sdsm_post_background_multi");
}

extern "C" int sdsm_post_fill_holes(int n, const int32_t *d_dims, const int64_t *d_off, const uint32_t *d_in, uint32_t *d_out, uint32_t *d_ws,
                                    const int64_t *d_ws_off, int32_t *d_status, void *stream)
{
    if (n < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_fill_holes: negative window count");
    if (n == 0) return SDSM_OK;
    if (!d_dims || !d_off || !d_in || !d_out || !d_status) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_fill_holes: null argument");
    if ((d_ws == nullptr) != (d_ws_off == nullptr)) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_fill_holes: workspace and its offsets go together");
    hipError_t e = sdsm_launch_post_fill(n, d_dims, d_off, d_in, d_out, d_ws, d_ws_off, d_status, (hipStream_t)stream);
    SET_DONE("sdsm_post_fill_holes");
}

extern "C" int sdsm_post_glare_multi(const sdsm_post_image *images, int n_images, const int32_t *d_boxes, const int64_t *d_bits_off,
                                     const uint32_t *d_bits, const double *h_props, int num_layers, uint32_t *d_ws, const int64_t *d_ws_off,
                                     int32_t *d_out, void *stream)
{
    SET_TABLE("sdsm_post_glare_multi", SET_SIDES);
    if (num_layers < 1 || num_layers > SDSM_POST_MAX_GLARE_LAYERS || !h_props) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_glare_multi: 1 <= num_layers <= 32 proportions required");
    int64_t n = 0;
    for (int j = 0; j < n_images; j++) {
        const sdsm_post_image &im = images[j];
        if (im.n_objects < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_glare_multi: negative object count");
        if (im.n_objects > 0 && !im.d_g) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_glare_multi: null image input");
        n += im.n_objects;
    }
    if (n >= INT_MAX) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_glare_multi: more than 2^31 - 1 objects");
    if (n == 0) return SDSM_OK;
    if (!d_boxes || !d_bits_off || !d_bits || !d_out) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_glare_multi: null argument");
    if ((d_ws == nullptr) != (d_ws_off == nullptr)) return fail(SDSM_ERR_ARGUMENT, "sdsm_post_glare_multi: workspace and its offsets go together");
    hipError_t e = sdsm_launch_post_glare(images, n_images, d_boxes, d_bits_off, d_bits, h_props, num_layers, d_ws, d_ws_off, d_out, (hipStream_t)stream);
    SET_DONE("sdsm_post_glare_multi");
}
