// Host side of a launch, shared by sdsm_plan.hip (plan, layout), sdsm_api.hip (entry points), sdsm_setup.hip and sdsm_solve.hip (launches): the
// launch lists of a plan, the zeroed words of a launch, the limits of the setup classes, the streams a launch runs on.  Each format is defined
// here and nowhere else (the workspace itself: the table of sdsm_plan.h).
#pragma once
#include <cstddef>
#include "sdsm_common.h"

// ---- launch lists ---------------------------------------------------------------------------------------------------------------
// A plan's `order` array holds seven lists one behind the other (layout_plan lays them out, sdsm_batch_upload copies them to the workspace).
struct ListSpan { int32_t first, count; };
struct LaunchLists {
    ListSpan all;             // every candidate, largest first: class 1 and the setup kernel of a one-launch setup
    ListSpan beyond_1;        // candidates whose bound on M admits more than class 1: classes 1b and 2 (upper bounds; most belong to class 1 after all)
    ListSpan beyond_2;        // ... more than class 2: class 2b and the global-memory class
    ListSpan group_members;   // (candidate | member << 24) of the workgroup groups
    ListSpan row_members;     // (candidate | member << 24) of sdsm_k_setup_rows
    ListSpan setup_small;     // setup in two launches (plans that mix small and large regions): the regions the 256-thread class sets up,
    ListSpan setup_big;       //   and the others; both empty in a one-launch setup
    bool forks() const { return beyond_1.count > 0 || beyond_2.count > 0 || group_members.count > 0; }   // some class runs beside class 1, on a side stream
};
static_assert(sizeof(LaunchLists) == 14 * sizeof(int32_t), "sdsm_plan_lists hands the spans out as int32[14]");

// The parameters of a kernel that walks one list.  P: the plan's parameters (make_params: `order` at the start of the array).
static inline BatchParams list_view(const BatchParams &P, ListSpan s)
{
    BatchParams V = P;
    V.order = P.order + s.first; V.n = s.count;
    return V;
}

// ---- launch words ---------------------------------------------------------------------------------------------------------------
// The block of the workspace that is zeroed before every launch.  The device reaches it through BatchParams.wide_ticket (ticket),
// BatchParams.cls_count (list_head) and cls_count + SDSM_SOLVER_COUNTERS (counters).
enum SolveList { LIST_1B = 0, LIST_2 = 1, LIST_2B = 2, LIST_3 = 3, LIST_1 = 4 };        // list_head[]: next entry of the launch list that a resident workgroup of the class takes
enum GroupTicket { TICKET_WIDE = 0, TICKET_WIDE2B = 1, TICKET_LIGHT = 2 };              // ticket[]: next entry of the group-member list, per group layout (class 2 / class 2b / light)
struct LaunchWords {
    int32_t ticket[16];
    int32_t list_head[32];
    unsigned long long counters[8];                   // [0] evaluations served from the kept sums (sdsm_batch_solver_counters)
};
static_assert(sizeof(LaunchWords) == 256 && offsetof(LaunchWords, ticket) == 0 && offsetof(LaunchWords, list_head) == 64 && offsetof(LaunchWords, counters) == 192, "layout of the launch words");
static_assert(offsetof(LaunchWords, counters) == offsetof(LaunchWords, list_head) + 4 * SDSM_SOLVER_COUNTERS, "the solve kernels find the counters at cls_count + SDSM_SOLVER_COUNTERS");

__host__ __device__ constexpr int group_ticket(int cls) { return cls == SDSM_CLS_WIDE_LIGHT ? TICKET_LIGHT : cls == SDSM_CLS_WIDE2B ? TICKET_WIDE2B : TICKET_WIDE; }
// What the gate of class 1 (sdsm_k_gate) watches, as its arguments encode it: a list head as it is, a group ticket as -1 - ticket.
constexpr int gate_list(SolveList l) { return l; }
constexpr int gate_ticket(GroupTicket t) { return -1 - t; }

// ---- setup classes --------------------------------------------------------------------------------------------------------------
// Limits of the setup kernel's LDS tables (sdsm_setup.hip): the plan picks the smallest class that holds it (sdsm_setup_class).
struct SetupLimS { static constexpr int DIM = 512, GRID = 512, PSFW = 1152, LABELS = 32767, WPE = 4, WG = 256, STATE = 22528; };      // 18 KB of tables (PSF k <= 33) + 22 KB for the state of a region in LDS (STATE bytes, sdsm_setup.hip RegionArrays): 40 KB
struct SetupLimM { static constexpr int DIM = 1024, GRID = 1024, PSFW = SDSM_PSF_LDS, LABELS = SDSM_MAX_LABELS, WPE = 4, WG = 1024, STATE = 0; };   // 37 KB: PSF k <= 65; plans with regions this large have few candidates: 1024 threads each
struct SetupLimL { static constexpr int DIM = SDSM_MAX_BBOX_DIM, GRID = SDSM_MAX_GRID, PSFW = SDSM_PSF_LDS, LABELS = SDSM_MAX_LABELS, WPE = 4, WG = 1024, STATE = 0; };   // 54 KB
constexpr bool sdsm_setup_fits_small(int h, int w, int mcap, int max_label, int k)
{
    return h <= SetupLimS::DIM && w <= SetupLimS::DIM && mcap <= SetupLimS::GRID && max_label <= SetupLimS::LABELS && k * k <= SetupLimS::PSFW;
}
constexpr int sdsm_setup_class(int max_dim, int max_mcap, int max_label, int k)
{
    return sdsm_setup_fits_small(max_dim, max_dim, max_mcap, max_label, k) ? 0 : max_dim <= SetupLimM::DIM && max_mcap <= SetupLimM::GRID ? 1 : 2;
}

// ---- streams and results of a launch --------------------------------------------------------------------------------------------
// side[0]: the global-memory class and class 2b; side[1]: the groups and class 2; side[2]: class 1b; side[3]: class 2b of plans without groups, or null
// (sdsm_launch_solve).  ev: five events owned by the side set: [0] the fork, [1 + i] the join of side i.  All null in a launch that does not fork.
struct LaunchStreams { hipStream_t caller; hipStream_t side[4]; hipEvent_t *ev; };
struct SolveOutputs { sdsm_record *records; uint32_t *masks; double *xi; };

extern "C" hipError_t sdsm_launch_setup(const BatchParams &P, hipStream_t stream, const LaunchLists &lists, int setup_class);
extern "C" hipError_t sdsm_launch_setup_rows(const BatchParams &P, hipStream_t stream, ListSpan row_members);
extern "C" hipError_t sdsm_launch_solve(const BatchParams &P, const SolveOutputs &out, const LaunchStreams &streams, const LaunchLists &lists);
