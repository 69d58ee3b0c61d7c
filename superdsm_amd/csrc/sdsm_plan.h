// The plan of a batch (sdsm_plan.hip): its candidates, launch lists and workspace.  Pure host arithmetic: the unit makes no HIP runtime call and
// links alone (tests/host/plan_check.cpp).  This header also holds the ONE definition of the workspace: the table of its blocks below.
#pragma once
#include <algorithm>
#include <climits>
#include <string>
#include <type_traits>
#include <vector>

#include "sdsm_launch.h"

#define SDSM_INTERNAL __attribute__((visibility("hidden")))

// The error text of the calling thread (sdsm_last_error), owned by sdsm_plan.hip.  Returns `code`.
SDSM_INTERNAL int fail(int code, const std::string &msg);

// ---- the workspace ----------------------------------------------------------------------------------------------------------------
// Every device buffer that the setup and solve kernels index, in the order they lie in the caller's workspace: X(field of BatchParams that
// the block is bound to, element type, elements -- an expression over the plan `p`).  Each block starts at a multiple of 256 bytes.  The
// offsets, the workspace size (layout_workspace), the typed pointers of the kernel arguments (make_params) and the values of
// sdsm_plan_layout all come from this table; the launch words (LaunchWords, zeroed before every launch) follow as the last block.
#define SDSM_WS_BLOCKS(X) \
    X(cand,      CandDesc,  std::max(p->n, 1)) \
    X(state,     CandState, std::max(p->n, 1)) \
    X(fp_labels, int32_t,   std::max<size_t>(p->fp_labels.size(), 1)) \
    X(order,     int32_t,   std::max<size_t>(p->order.size(), 1)) \
    X(psf,       float,     p->psf.size()) \
    X(crop_y,    double,    SDSM_RUN * std::max<int64_t>(p->total_runs, 1)) \
    X(crop_rc,   uint32_t,  std::max<int64_t>(p->total_runs, 1)) \
    X(run_meta,  uint32_t,  std::max<int64_t>(p->total_runs, 1)) \
    X(run_q0,    uint32_t,  std::max<int64_t>(p->total_runs, 1)) \
    X(run_aux,   uint32_t,  std::max<int64_t>(p->total_runs, 1)) \
    X(crop_cc,   uint32_t,  std::max<int64_t>(p->total_pixels, 1)) \
    X(dist,      uint32_t,  std::max<int64_t>(p->total_pixels, 1)) \
    X(tmp_y,     double,    std::max<int64_t>(p->total_pixels, 1)) \
    X(tmp_rc,    uint32_t,  std::max<int64_t>(p->total_pixels, 1)) \
    X(inv,       uint32_t,  std::max<int64_t>(p->total_pixels, 1)) \
    X(grid_rc,   uint32_t,  std::max<int64_t>(p->total_xi, 1)) \
    X(ell_im,    uint32_t,  std::max<int64_t>(p->total_ell, 1)) \
    X(ell_w,     float,     4 * std::max<int64_t>(p->total_ell, 1))     /* the weights of a run's four pixels per entry */ \
    X(env_fst,   int32_t,   std::max<int64_t>(p->total_xi, 1)) \
    X(env_rb,    int32_t,   std::max<int64_t>(p->total_xi, 1)) \
    X(hglob,     double,    std::max<int64_t>(p->n_hglob, 1)) \
    X(wide_pool, double,    std::max<int64_t>(p->n_wide, 1))
#define X(name, T, count) WS_##name,
enum WsBlock { SDSM_WS_BLOCKS(X) WS_words, WS_COUNT };
#undef X
#define X(name, T, count) static_assert(std::is_same<std::remove_cv_t<std::remove_pointer_t<decltype(BatchParams::name)>>, T>::value, "element type of workspace block " #name);
SDSM_WS_BLOCKS(X)
#undef X

struct PlanImage { int H, W, n_atoms; };
struct SideSet;                                 // the side streams of a device (sdsm_sides.h)

struct sdsm_plan {
    int n = 0;
    std::vector<PlanImage> images;             // one entry for sdsm_plan_create, several for sdsm_plan_create_multi
    sdsm_dsm_config cfg{};
    int k = 1, R = 0, zcap = 1, zcap_run = 1, zshift = 0, no_deform = 0;
    std::vector<CandDesc> cand;
    std::vector<int32_t> fp_labels, order;     // order: the launch lists, one behind the other
    LaunchLists lists{};                        // where each of them is (layout_plan)
    int rows_mcap = 1;                          // largest bound on M among the regions of the list of row members
    int max_label = 1;
    int setup_class = 2;         // LDS limits of the setup kernel that hold this plan (sdsm_setup_class)
    int mode = 0;                // sdsm_plan_set_latency_mode: 0 throughput, 1 latency, 2 no workgroup groups
    int wide_pixels = INT_MAX;   // throughput mode by default
    int boost_pixels = INT_MAX;  // regions above run their pixel passes at a raised priority (throughput mode, layout_plan)
    int wide_rest = 0;           // some group's bound on M admits more unknowns than the layout of class 2b holds (layout_plan; see sdsm_launch_solve)
    std::vector<float> psf;
    std::vector<int32_t> mask_info, n_pixels;
    std::vector<int64_t> mask_off_bytes, xi_off;
    int64_t total_pixels = 0, total_runs = 0, total_ell = 0, total_xi = 0, total_mask_words = 0, n_hglob = 0, n_wide = 0;   // n_hglob, n_wide count doubles
    size_t ws_off[WS_COUNT] = {}, total = 0;   // byte offset of every block of the workspace, and its size (layout_workspace)
    // The launch lists and CandDesc.wide_* live in the workspace (sdsm_batch_upload): a layout change after the upload
    // (sdsm_plan_set_latency_mode) would leave stale tables on the device, so launches check the generation they were uploaded at.
    uint64_t layout_gen = 0;
    mutable const double *x0 = nullptr;   // sdsm_plan_set_start: device pointer to the starting points of the DSM solves, or null
    mutable uint64_t uploaded_gen = 0;
    mutable const void *uploaded_ws = nullptr;
    // side streams / fork-join events of the solve classes, borrowed from the device's set at the plan's first launch (sdsm_sides.hip)
    mutable SideSet *sides = nullptr;
};

// Kernel arguments of a plan laid out in the caller's workspace: the typed pointer of every block of the table, the scalars, the process-wide
// diagnostic settings.  The image pointers are left null (the launch binds them).  A null workspace gives every block's offset.
SDSM_INTERNAL BatchParams make_params(const sdsm_plan *p, void *d_ws);
// The launch words of the plan in a workspace.
static inline LaunchWords *ws_words(const sdsm_plan *p, void *d_ws) { return (LaunchWords *)((uintptr_t)d_ws + p->ws_off[WS_words]); }
