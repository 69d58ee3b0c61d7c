// Host side of the C ABI (include/sdsm.h): planning, workspace layout, launches.  No device allocation
// happens here: every device buffer is provided by the caller.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "sdsm_launch.h"
#include <climits>

extern "C" hipError_t sdsm_image_prepare_impl(const double *, const uint8_t *, const int32_t *, int, int, double, int, uint8_t *, int32_t *, void *, hipStream_t);
extern "C" hipError_t sdsm_preprocess_impl(const double *, int, int, double, double, double, int, double *, void *, hipStream_t);
extern "C" void sdsm_gauss_kernel_host(double sigma, int radius, double *w);
extern "C" int sdsm_setup_fits_small(int h, int w, int mcap, int max_label, int k);
extern "C" int sdsm_setup_class(int max_dim, int max_mcap, int max_label, int k);

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
static int hipfail(hipError_t e, const char *what) { return fail(SDSM_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" int sdsm_version(void) { return SDSM_VERSION; }
extern "C" const char *sdsm_last_error(void) { return g_err.c_str(); }

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

// ---- PSF of G~ (dsm.py:137-142): delta image filtered with SciPy's gaussian_filter, float32 ----------
static inline long reflect_h(long i, long n) { long p = 2 * n, m = i % p; if (m < 0) m += p; return m < n ? m : p - 1 - m; }

static void correlate_line(const double *in, long n, long stride, const double *w, int R, double *out)
{
    std::vector<double> buf(n + 2 * R);
    for (long i = -R; i < n + R; i++) buf[i + R] = in[reflect_h(i, n) * stride];
    for (long l = 0; l < n; l++) {
        const double *c = buf.data() + l + R;
        double acc = c[0] * w[R];
        for (int j = R; j >= 1; j--) acc += (c[-j] + c[j]) * w[R - j];
        out[l * stride] = acc;
    }
}

static int make_psf(double sigma, double mult, std::vector<float> &psf)
{
    int k = (int)std::nearbyint(1 + sigma * 4 * mult);
    if (k < 1) k = 1;
    int R = (int)(4.0 * sigma + 0.5);
    std::vector<double> w(2 * R + 1), a((size_t)k * k, 0.0), b((size_t)k * k), c((size_t)k * k);
    sdsm_gauss_kernel_host(sigma, R, w.data());
    a[(size_t)(k / 2) * k + k / 2] = 1;
    for (int col = 0; col < k; col++) correlate_line(a.data() + col, k, k, w.data(), R, b.data() + col);
    for (int row = 0; row < k; row++) correlate_line(b.data() + (size_t)row * k, k, 1, w.data(), R, c.data() + (size_t)row * k);
    psf.resize((size_t)k * k);
    for (size_t i = 0; i < psf.size(); i++) psf[i] = (float)c[i];
    return k;
}

extern "C" int sdsm_psf(double sigma, double multiplier, float *out)
{
    if (!(sigma > 0) || std::isinf(sigma)) return fail(SDSM_ERR_ARGUMENT, "sdsm_psf: sigma must be finite and positive");
    std::vector<float> psf;
    int k = make_psf(sigma, multiplier, psf);
    if (out) memcpy(out, psf.data(), psf.size() * sizeof(float));
    return k;
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

// ---- plan ------------------------------------------------------------------------------------------------
struct PlanImage { int H, W, n_atoms; };

// Side streams / fork-join events of the solve classes.  A plan borrows a set at its first launch and gives it back when it is
// destroyed: creating and destroying HIP streams costs milliseconds (hipStreamDestroy synchronises), a reference-style caller
// builds a plan per batch.  A set carries no state between users (events are recorded before they are waited for).
// The set holds a POOL of side streams, created on demand, and for every caller stream it has seen the pool streams that run side by side
// with that stream and with each other (choose_sides): which hardware queue a stream lands on depends on every stream the process
// created before it, so no fixed set of streams is clear of every caller's queue.
#include <atomic>
#include <mutex>
// state of a choice: 1 the caller's stream and the sides run side by side, 0 fewer than three clean sides (classes share a queue), -1 a probe stayed undecided
struct SideChoice { hipStream_t caller = nullptr; int idx[4] = {-1, -1, -1, -1}; int want = 0, clean = 0, state = 0, reprobes = 0; uint64_t born = 0; bool valid = false; };
struct SideSet {
    hipStream_t pool[SDSM_SIDE_POOL]; int n_pool = 0; hipEvent_t fj[5]; int device; std::mutex enqueue;
    int32_t *probe_words = nullptr;                 // SDSM_PROBE_BYTES, allocated once
    SideChoice cache[SDSM_SIDE_CACHE]; uint64_t tick = 0; int probes = 0, unknowns = 0; bool warned = false;
};
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
    int64_t total_pixels = 0, total_runs = 0, total_ell = 0, total_xi = 0, total_mask_words = 0, n_hglob = 0, n_wide = 0;
    size_t off_cand = 0, off_state = 0, off_fp = 0, off_order = 0, off_crop_y = 0, off_crop_rc = 0, off_crop_cc = 0, off_dist = 0, off_tmp_y = 0, off_tmp_rc = 0, off_inv = 0, off_run_meta = 0,
           off_run_q0 = 0, off_run_aux = 0, off_grid = 0, off_ell_im = 0, off_ell_w = 0, off_psf = 0, off_env_fst = 0, off_env_rb = 0, off_hglob = 0, off_wide = 0, off_words = 0, total = 0;
    // The launch lists and CandDesc.wide_* live in the workspace (sdsm_batch_upload): a layout change after the upload
    // (sdsm_plan_set_latency_mode) would leave stale tables on the device, so launches check the generation they were uploaded at.
    uint64_t layout_gen = 0;
    mutable const double *x0 = nullptr;   // sdsm_plan_set_start: device pointer to the starting points of the DSM solves, or null
    mutable uint64_t uploaded_gen = 0;
    mutable const void *uploaded_ws = nullptr;
    // side streams / fork-join events of the solve classes, owned by the plan (created at its first launch)
    mutable SideSet *sides = nullptr;
};

#include <mutex>
// ONE set per device, shared by all plans and created at the first launch that needs it: the runtime maps streams onto GPU_MAX_HW_QUEUES
// hardware queues in the order of their creation, and side streams created per live plan (the tenth stream of the process and later) came to share
// queues with the caller's stream or among themselves -- the classes of one launch then ran one after the other (NIH3T3-like launch inside the full
// bench run 8.3 instead of 6.4 ms).  One fixed set is no better off once the caller has streams of its own (the step of 8 different images from a
// stream of PyTorch's pool: classes 1b and 2 on one queue, 10.1 instead of 6.4 ms): hence the pool and the choice per caller stream below.
// Launches enqueue under the set's mutex (fork and join events belong to the set); launches from different caller streams share the pool.
static std::mutex g_pool_mutex;
static std::atomic<int> g_light_emax{-1};   // sdsm_set_light_envelope_limit (process-wide): -1 = the rule of light_limit()
static std::vector<SideSet *> g_side_sets;

static hipError_t acquire_sides(const sdsm_plan *p, hipStream_t caller)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    // the set belongs to a device: the caller's stream must live on the calling thread's current device (as PyTorch arranges it) -- a stream of another device
    // would fork work onto side streams of the wrong card
    int sdev = dev;
    if (caller && hipStreamGetDevice(caller, &sdev) == hipSuccess && sdev != dev) return hipErrorInvalidDevice;
    (void)hipGetLastError();
    if (p->sides) return p->sides->device == dev ? hipSuccess : hipErrorInvalidDevice;   // (a plan stays with the device of its first launch)
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    for (SideSet *q : g_side_sets) if (q->device == dev) { p->sides = q; return hipSuccess; }
    SideSet *s = new SideSet();
    s->device = dev;
    // (the streams of the pool are created when a caller stream needs them: grow_pool)
    for (int i = 0; i < 5; i++) if ((e = hipEventCreateWithFlags(&s->fj[i], hipEventDisableTiming)) != hipSuccess) { delete s; return e; }
    g_side_sets.push_back(s);
    p->sides = s;
    return hipSuccess;
}

static size_t al(size_t v) { return (v + 255) / 256 * 256; }

// Multiplier A ~ 0.618 N coprime to N defines the scatter "position q holds raster rank (q * A) mod N"; the setup
// kernel needs the inverse map rank -> position, i.e. A^-1 mod N.
static uint32_t perm_inverse(uint32_t N)
{
    if (N <= 2) return 1;
    uint64_t A = (uint64_t)(0.6180339887498949 * N);
    if (A < 1) A = 1;
    auto gcd = [](uint64_t a, uint64_t b) { while (b) { uint64_t t = a % b; a = b; b = t; } return a; };
    while (gcd(A, N) != 1) A++;
    // extended Euclid: A * x = 1 (mod N)
    int64_t t = 0, newt = 1, r = N, newr = (int64_t)(A % N);
    while (newr != 0) { int64_t q = r / newr; int64_t tmp = t - q * newt; t = newt; newt = tmp; tmp = r - q * newr; r = newr; newr = tmp; }
    if (t < 0) t += N;
    return (uint32_t)t;
}

#ifndef SDSM_LAT_SLICE
#define SDSM_LAT_SLICE 2048         // latency mode: pixels per member of the group of a mid-size region
#endif
#ifndef SDSM_LAT_GMAX
#define SDSM_LAT_GMAX 4
#endif
#ifndef SDSM_ROWS_MAX_REGIONS
#define SDSM_ROWS_MAX_REGIONS 1024     // plans with more regions above SDSM_ROWS_MIN_PIXELS build all rows in the setup kernel
#endif
#ifndef SDSM_WIDE_TP_MIN_PIXELS
#define SDSM_WIDE_TP_MIN_PIXELS 8192   // throughput mode: no groups below this many pixels
#endif
#ifndef SDSM_K1_PIXDIV
#define SDSM_K1_PIXDIV 2048             // throughput mode: regions above (pixels of all candidates) / SDSM_K1_PIXDIV pixels leave the 192 / 256-thread classes
#endif
#ifndef SDSM_WIDE_FILL
#define SDSM_WIDE_FILL 1024              // throughput mode: groups only for regions of more than (pixels of all candidates) / SDSM_WIDE_FILL pixels
#endif
#ifndef SDSM_WIDE_MAX_MEMBERS
#define SDSM_WIDE_MAX_MEMBERS 256    // throughput mode: group members of one launch (= compute units of an MI355X); the largest regions first
#endif
// Throughput mode: the grouped regions that END a launch get members beyond one per SDSM_WIDE_SLICE pixels -- those that may not be light (their bound on M
// exceeds the light class's unknowns, so they keep a compute unit per member whatever they get) and have at least SDSM_WIDE_BONUS_PCT per cent of the pixels
// of the plan's largest grouped region.  A member more shortens the passes over the pixels and costs a compute unit.
#ifndef SDSM_WIDE_BONUS
#define SDSM_WIDE_BONUS 1            // members more (0: the rule is off; 1 and 2 at 90 %, 1 at 60 % measured on the 8-image step: DESIGN section 9 (z))
#endif
#ifndef SDSM_WIDE_BONUS_PCT
#define SDSM_WIDE_BONUS_PCT 90
#endif
// Envelope limit of the light group class for a plan's launches (0: none).  A class-1 slot beside a group member only helps a launch whose class-1 candidates
// outnumber the class-1 workgroups the chip holds (about 1000, r04_occupancy_probe): in a smaller plan every candidate has a slot at once and the light members
// would only pay for their third wavefront per SIMD (they run 7-19 % longer; NIH3T3-like, 234 candidates: 5.75 -> 5.89 ms per launch with light groups).
// An explicit limit (sdsm_set_light_envelope_limit, tests) holds for every plan with groups.
#ifndef SDSM_LIGHT_MIN_CANDIDATES
#define SDSM_LIGHT_MIN_CANDIDATES 1024
#endif
// Workgroup groups, launch lists and workspace layout (repeated when the scheduling mode changes).
static int light_limit(const sdsm_plan *p)
{
    if (!SDSM_LIGHT_GROUPS || p->lists.group_members.count <= 0) return 0;
    const int v = g_light_emax.load(std::memory_order_relaxed);
    if (v >= 0) return v;
    return p->n > SDSM_LIGHT_MIN_CANDIDATES ? SDSM_KL_EMAX : 0;
}
static void layout_plan(sdsm_plan *p)
{
    const int n = p->n;
    const bool latency = p->mode == 1, groups = p->mode != 2;
    p->wide_pixels = latency ? SDSM_WIDE_PIXELS : INT_MAX;
    p->boost_pixels = INT_MAX;
    p->layout_gen++;
    p->n_wide = 0;
    // Groups shorten the longest chains of a launch; every member holds a whole compute unit and a group only advances while all of its
    // members are resident.  In throughput mode the LARGEST regions get groups until their members add up to the compute units of the
    // chip; very large regions beyond that (synthetic 4096^2 image: 434 of them, 1296 members -- they waited for each other behind the
    // small classes) are solved as ordinary class-2 candidates, one workgroup each.
    long long wide_thr = SDSM_WIDE_MIN_PIXELS;       // regions with more pixels get a group of one member per SDSM_WIDE_SLICE pixels (throughput mode: set below)
    if (groups && !latency) {
        // ... and only regions whose chain (~ its pixels) is long next to the time the whole plan keeps the chip busy (~ all pixels / compute units):
        // the synthetic 4096^2 plan (10 073 candidates, 50 M pixels) gets no groups at all -- its 31 k-pixel regions end long before the rest does,
        // and groups there cost compute units that the other candidates wait for (75 -> 97 ms with groups for everything above 12 288 pixels)
        long long all_pixels = 0;
        for (int i = 0; i < n; i++) all_pixels += p->cand[i].N;
        long long tp_min = SDSM_WIDE_TP_MIN_PIXELS;
        if (const char *e = getenv("SDSM_WIDE_TP_MIN_PIXELS")) { const long long v = atoll(e); if (v > 0) tp_min = v; }   // diagnostic knob
        wide_thr = std::max<long long>(tp_min, all_pixels / SDSM_WIDE_FILL);
    }
    if (!latency) {
        // Throughput mode: a candidate whose chain (~ its pixels) is long next to the time the plan keeps the chip busy (~ pixels of all
        // candidates / 1024 workgroup slots of class 1) runs its passes over the pixels at a raised issue priority: regions above 1 /
        // SDSM_K1_PIXDIV of all pixels.  8 different BBBC039-like images: class 1 took 6.8 ms beside the other classes while its workgroup
        // time was 3.6 ms of the chip -- its 4-5 ms chains (6-7 k pixels, 95-114 unknowns; 2.8 ms on an idle chip) ended it.  (Moving
        // them to the 512-thread classes instead, a compute unit each: 7.6 -> 8.7-9.2 ms per step, measured in round 4.)
        long long all_pixels = 0;
        for (int i = 0; i < n; i++) all_pixels += p->cand[i].N;
        long long div = SDSM_K1_PIXDIV;
        if (const char *e = getenv("SDSM_K1_PIXDIV")) { const long long v = atoll(e); if (v > 0) div = v; else if (v < 0) div = 0; }   // diagnostic knob (negative: no bound)
        p->boost_pixels = div > 0 ? (int)std::min<long long>(INT_MAX, std::max<long long>(SDSM_WIDE_PIXELS, all_pixels / div)) : INT_MAX;
    }
    long wide_slice = SDSM_WIDE_SLICE;
    if (const char *e = getenv("SDSM_WIDE_SLICE")) { const long v = atol(e); if (v > 0) wide_slice = v; }                // diagnostic knob
    auto group_size = [&](long N) -> long {              // members of the group a region of N pixels would get (0: none)
        if (!groups || n >= (1 << 24)) return 0;
        if (N > wide_thr) return std::min<long>(SDSM_WIDE_MAX_G, std::max<long>(2, (N + wide_slice - 1) / wide_slice));
        if (latency && N > SDSM_WIDE_PIXELS) return std::min<long>(SDSM_LAT_GMAX, std::max<long>(2, (N + SDSM_LAT_SLICE - 1) / SDSM_LAT_SLICE));   // latency mode: the largest regions of an ordinary image too
        return 0;
    };
    // the member budget (both modes: a single image with many large clusters -- 636 candidates, 16 k-pixel regions -- asked for several hundred
    // members in latency mode and took 15 ms instead of 12)
    std::vector<char> grouped(n, 1), bonus(n, 0);
    {
        std::vector<int> big;
        for (int i = 0; i < n; i++) if (group_size(p->cand[i].N) > 0) big.push_back(i);
        std::stable_sort(big.begin(), big.end(), [&](int a, int b) { return p->cand[a].N > p->cand[b].N; });
        long members = 0;
        int cutoff = 0;                                  // regions of at most this many pixels get no group (equal regions are treated alike)
        for (int i : big) {
            members += group_size(p->cand[i].N);
            if (members > SDSM_WIDE_MAX_MEMBERS) { cutoff = p->cand[i].N; break; }
        }
        for (int i : big) if (p->cand[i].N <= cutoff) grouped[i] = 0;
        // the bonus members, inside the same budget, the largest regions first
        if (SDSM_WIDE_BONUS > 0 && groups && !latency) {
            long used = 0, nmax = 0;
            for (int i : big) if (grouped[i]) { used += group_size(p->cand[i].N); nmax = std::max<long>(nmax, p->cand[i].N); }
            for (int i : big) {
                if (!grouped[i] || 6 + (long)p->cand[i].Mcap <= SDSM_KL_NMAX || (long long)p->cand[i].N * 100 < (long long)nmax * SDSM_WIDE_BONUS_PCT) continue;
                const long g = group_size(p->cand[i].N);
                const long b = std::min<long>(std::min<long>(SDSM_WIDE_BONUS, SDSM_WIDE_MAX_G - g), SDSM_WIDE_MAX_MEMBERS - used);
                if (b > 0) { bonus[i] = (char)b; used += b; }
            }
        }
    }
    long rows_regions = 0;
    for (int i = 0; i < n; i++) rows_regions += p->cand[i].N > SDSM_ROWS_MIN_PIXELS;
    const bool rows_multi = rows_regions <= SDSM_ROWS_MAX_REGIONS;
    for (int i = 0; i < n; i++) {
        CandDesc &c = p->cand[i];
        const long G = grouped[i] ? group_size(c.N) + bonus[i] : 0;
        // rows of G~ by several workgroups for every large region, whether or not a workgroup group solves it (a 12 k-pixel region took a
        // single setup workgroup 0.5-1 ms: the end of the setup kernel)
        // (only while such regions are few enough to be the END of the setup kernel: with the 5000 of the synthetic 4096^2 plan the setup kernel is
        // busy throughout and builds the rows itself at a little more than half the cost -- 5.2 instead of 9.2 ms there)
        const long RG = rows_multi && c.N > SDSM_ROWS_MIN_PIXELS && n < (1 << 24) ? std::min<long>(SDSM_ROWS_MAX_G, (c.N + SDSM_ROWS_SLICE - 1) / SDSM_ROWS_SLICE) : 0;
        c.rows_g = (int32_t)std::max<long>(RG, G > 0 ? 1 : 0);
        c.pad1 = 0;
        c.wide_g = (int32_t)G;
        if (G > 0 || c.rows_g > 0) { c.wide_off = p->n_wide; p->n_wide += SDSM_WIDE_SYNC + (int64_t)2 * G * SDSM_WIDE_PBUF; }
        else c.wide_off = -1;
    }
    p->wide_rest = 0;
    for (int i = 0; i < n; i++) if (p->cand[i].wide_g > 0 && 6 + (long)p->cand[i].Mcap > SDSM_K2B_NMAX) p->wide_rest = 1;
    p->rows_mcap = 1;
    std::vector<int32_t> all(n), beyond_1, beyond_2, group_members, row_members, setup_small, setup_big;
    std::iota(all.begin(), all.end(), 0);
    std::stable_sort(all.begin(), all.end(), [&](int a, int b) { return p->cand[a].N > p->cand[b].N; });
    // a candidate can only belong to a larger size class if its upper bound Mcap allows it: the larger classes get
    // their own (shorter) launch lists instead of n workgroups that exit immediately
    for (int ci : all) if (6 + p->cand[ci].Mcap > SDSM_K1_DENSE_N || p->cand[ci].N > SDSM_WIDE_PIXELS) beyond_1.push_back(ci);
    for (int ci : all) if (6 + p->cand[ci].Mcap > SDSM_ENV_DENSE_N) beyond_2.push_back(ci);
    for (int ci : all) for (int g = 0; g < p->cand[ci].wide_g; g++) group_members.push_back(ci | (g << 24));
    for (int ci : all) {
        for (int g = 0; g < p->cand[ci].rows_g; g++) row_members.push_back(ci | (g << 24));
        if (p->cand[ci].rows_g > 0) p->rows_mcap = std::max(p->rows_mcap, (int)std::min<int64_t>(p->cand[ci].Mcap, SDSM_MAX_N_GLOBAL));
    }
    // Setup: a plan whose largest region needs the large tables of the setup kernel (1024 threads per candidate) but whose candidates are
    // mostly small (an image set with a few big clusters) sets the small ones up with the 256-thread class in a launch of its own
    if (p->setup_class != 0) {
        for (int ci : all) {
            const CandDesc &c = p->cand[ci];
            (c.N <= SDSM_SETUP_SMALL_PIXELS && sdsm_setup_fits_small(c.h, c.w, c.Mcap, p->max_label, p->k) ? setup_small : setup_big).push_back(ci);
        }
        if (setup_small.size() < 256) { setup_small.clear(); setup_big.clear(); }
    }
    // the one place that lays the lists out in `order` (the initialisers run left to right)
    p->order.clear();
    auto put = [&](const std::vector<int32_t> &list) { const ListSpan at{(int32_t)p->order.size(), (int32_t)list.size()}; p->order.insert(p->order.end(), list.begin(), list.end()); return at; };
    p->lists = LaunchLists{put(all), put(beyond_1), put(beyond_2), put(group_members), put(row_members), put(setup_small), put(setup_big)};
    // workspace layout
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += al(bytes); return r; };
    p->off_cand = take(sizeof(CandDesc) * std::max(n, 1));
    p->off_state = take(sizeof(CandState) * std::max(n, 1));
    p->off_fp = take(4 * std::max<size_t>(p->fp_labels.size(), 1));
    p->off_order = take(4 * std::max<size_t>(p->order.size(), 1));
    p->off_psf = take(4 * p->psf.size());
    size_t np = (size_t)std::max<int64_t>(p->total_pixels, 1), nr = (size_t)std::max<int64_t>(p->total_runs, 1);
    p->off_crop_y = take(8 * SDSM_RUN * nr);
    p->off_crop_rc = take(4 * nr);
    p->off_run_meta = take(4 * nr);
    p->off_run_q0 = take(4 * nr);
    p->off_run_aux = take(4 * nr);
    p->off_crop_cc = take(4 * np);
    p->off_dist = take(4 * np);
    p->off_tmp_y = take(8 * np);
    p->off_tmp_rc = take(4 * np);
    p->off_inv = take(4 * np);
    p->off_grid = take(4 * (size_t)std::max<int64_t>(p->total_xi, 1));
    p->off_ell_im = take(4 * (size_t)std::max<int64_t>(p->total_ell, 1));
    p->off_ell_w = take(16 * (size_t)std::max<int64_t>(p->total_ell, 1));
    p->off_env_fst = take(4 * (size_t)std::max<int64_t>(p->total_xi, 1));
    p->off_env_rb = take(4 * (size_t)std::max<int64_t>(p->total_xi, 1));
    p->off_hglob = take(8 * (size_t)std::max<int64_t>(p->n_hglob, 1));      // n_hglob counts doubles
    p->off_wide = take(8 * (size_t)std::max<int64_t>(p->n_wide, 1));        // n_wide counts doubles
    p->off_words = take(sizeof(LaunchWords));                                 // zeroed before every launch
    p->total = o;
}
extern "C" sdsm_plan *sdsm_plan_create_multi(int n_images, const int32_t *H, const int32_t *W, const int32_t *n_atoms, const int32_t *const *atom_stats,
                                             const sdsm_dsm_config *cfg, int n, const int32_t *offsets, const int32_t *labels, const int32_t *image_of)
{
    if (n_images < 1 || n_images > SDSM_MAX_IMAGES || !H || !W || !n_atoms || !atom_stats || !cfg || n < 0 || (n > 0 && (!offsets || !labels)) || (n > 0 && n_images > 1 && !image_of)) {
        fail(SDSM_ERR_ARGUMENT, "sdsm_plan_create: bad argument (1 .. 16 images per plan)"); return nullptr;
    }
    for (int i = 0; i < n_images; i++) if (H[i] < 2 || W[i] < 2 || !atom_stats[i] || n_atoms[i] < 0) { fail(SDSM_ERR_ARGUMENT, "sdsm_plan_create: bad image"); return nullptr; }
    if (!(cfg->epsilon > 0) || !(cfg->alpha >= 0) || !(cfg->scale > 0) || cfg->smooth_subsample < 1 || !(cfg->smooth_amount > 0)) {
        fail(SDSM_ERR_ARGUMENT, "sdsm_plan_create: epsilon > 0, alpha >= 0, scale > 0, smooth_subsample >= 1, smooth_amount > 0 required (dsm.py:275-285)");
        return nullptr;
    }
    sdsm_plan *p = new sdsm_plan();
    p->n = n; p->cfg = *cfg;
    for (int i = 0; i < n_images; i++) p->images.push_back({H[i], W[i], n_atoms[i]});
    if (p->cfg.max_iters <= 0) p->cfg.max_iters = 100;
    p->no_deform = std::isinf(cfg->smooth_amount) ? 1 : 0;
    if (!p->no_deform) {
        p->k = make_psf(cfg->smooth_amount, cfg->gaussian_shape_multiplier, p->psf);
        if (p->k % 2 == 0) {   // _convmat asserts an odd filter size (dsm.py:147)
            fail(SDSM_ERR_ARGUMENT, "sdsm_plan_create: round(1 + 4 * smooth_amount * gaussian_shape_multiplier) must be odd (dsm.py:147)");
            delete p; return nullptr;
        }
        p->R = p->k / 2;
        long per = (2 * p->R) / cfg->smooth_subsample + 1;
        long z = per * per;
        p->zcap = (int)std::min<long>(z, 4 * SDSM_MAX_ELL_GROUPS);   // grid points are at least `subsample` apart (chessboard): at most per^2 inside a pixel's window; a solvable row has <= M <= 1018 entries
        // a run spans up to SDSM_RUN columns: the union of its pixels' windows is SDSM_RUN - 1 columns wider
        const long per_c = (2 * p->R + SDSM_RUN - 1) / cfg->smooth_subsample + 1;
        p->zcap_run = (int)std::min<long>(per * per_c, 4 * SDSM_MAX_ELL_GROUPS);
        p->zshift = p->zcap_run > SDSM_MAX_ELL_GROUPS ? 2 : 0;
        if (p->zshift) p->zcap_run = (p->zcap_run + 3) / 4 * 4;                   // sort classes of 4 entries: rows are padded to whole classes
    } else { p->psf.assign(1, 1.f); p->k = 1; p->R = 0; p->zcap = 1; p->zcap_run = 1; p->zshift = 0; }
    const int s = cfg->smooth_subsample;
    p->cand.resize(n); p->mask_info.resize((size_t)4 * n); p->mask_off_bytes.resize(n); p->xi_off.resize(n); p->n_pixels.resize(n);
    p->fp_labels.assign(labels, labels + (n > 0 ? offsets[n] : 0));
    for (int i = 0; i < n; i++) {
        CandDesc &c = p->cand[i];
        const int im = image_of ? image_of[i] : 0;
        if (im < 0 || im >= n_images) { fail(SDSM_ERR_ARGUMENT, "sdsm_plan_create: image index out of range"); delete p; return nullptr; }
        const int Hi = H[im], Wi = W[im];
        long N = 0; int r0 = Hi, r1 = -1, c0 = Wi, c1 = -1;
        for (int e = offsets[i]; e < offsets[i + 1]; e++) {
            int l = labels[e];
            if (l < 1 || l > n_atoms[im]) continue;
            const int32_t *st = atom_stats[im] + (size_t)l * SDSM_ATOM_STATS_STRIDE;
            if (st[0] <= 0) continue;
            N += st[0];
            r0 = std::min(r0, st[1]); r1 = std::max(r1, st[2]); c0 = std::min(c0, st[3]); c1 = std::max(c1, st[4]);
        }
        if (r1 < 0) { r0 = c0 = 0; r1 = c1 = 0; N = 0; }
        c.image = im; c.pad1 = 0; c.rows_g = 0;
        c.N = (int32_t)N; c.r0 = r0; c.c0 = c0; c.h = r1 - r0 + 1; c.w = c1 - c0 + 1;
        c.fp_off = offsets[i]; c.fp_len = offsets[i + 1] - offsets[i];
        long mc = p->no_deform ? 1 : (long)((c.h + s - 1) / s) * ((c.w + s - 1) / s);
        c.Mcap = (int32_t)std::max<long>(1, std::min<long>(mc, std::max<long>(N, 1)));
        // runs: the region pixels of one image row inside one aligned 4-column cell; at most one per pixel and one per cell of the bounding box
        const long ncw = c.w > 0 ? ((c0 + c.w - 1) >> 2) - (c0 >> 2) + 1 : 1;
        c.NRcap = (int32_t)std::max<long>(1, std::min<long>(N, (long)c.h * ncw));
        c.crop_off = p->total_pixels; p->total_pixels += N;
        c.run_off = p->total_runs; p->total_runs += c.NRcap;
        c.ell_off = p->total_ell; p->total_ell += (int64_t)c.NRcap * p->zcap_run;
        c.xi_off = p->total_xi; p->total_xi += c.Mcap;
        c.mask_off = p->total_mask_words; p->total_mask_words += ((int64_t)c.h * c.w + 31) / 32;
        if (6 + c.Mcap > SDSM_ENV_DENSE_N) {
            const int64_t nn = 6 + std::min<int64_t>(c.Mcap, SDSM_MAX_N_GLOBAL - 6);
            c.hglob_off = p->n_hglob; p->n_hglob += nn * (nn + 1) / 2;
        } else c.hglob_off = -1;
        c.perm_inv = perm_inverse((uint32_t)std::max<long>(N, 1));
        p->mask_info[4 * i] = r0; p->mask_info[4 * i + 1] = c0; p->mask_info[4 * i + 2] = c.h; p->mask_info[4 * i + 3] = c.w;
        p->mask_off_bytes[i] = c.mask_off * 4; p->xi_off[i] = c.xi_off; p->n_pixels[i] = c.N;
    }
    {
        int max_dim = 1, max_mcap = 1, max_label = 1;
        for (const CandDesc &c : p->cand) { max_dim = std::max(max_dim, std::max(c.h, c.w)); max_mcap = std::max(max_mcap, c.Mcap); }
        for (int im = 0; im < n_images; im++) max_label = std::max(max_label, n_atoms[im]);
        p->setup_class = sdsm_setup_class(max_dim, max_mcap, max_label, p->k);
        p->max_label = max_label;
    }
    layout_plan(p);
    return p;
}

extern "C" sdsm_plan *sdsm_plan_create(int H, int W, int n_atoms, const int32_t *atom_stats, const sdsm_dsm_config *cfg,
                                       int n, const int32_t *offsets, const int32_t *labels)
{
    const int32_t h = H, w = W, na = n_atoms;
    return sdsm_plan_create_multi(1, &h, &w, &na, &atom_stats, cfg, n, offsets, labels, nullptr);
}

extern "C" void sdsm_plan_destroy(sdsm_plan *plan)
{
    if (!plan) return;
    delete plan;                                         // (the side streams belong to the device, not to the plan)
}
extern "C" int sdsm_plan_set_latency_mode(sdsm_plan *p, int on)
{
    if (!p) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_set_latency_mode: null plan");
    if (on < 0 || on > 2) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_set_latency_mode: mode must be 0, 1 or 2");
    p->mode = on;
    layout_plan(p);                                       // new launch lists / workspace size / generation: upload again before the next launch
    return SDSM_OK;
}
extern "C" size_t sdsm_plan_workspace_bytes(const sdsm_plan *p) { return p ? p->total : 0; }
extern "C" size_t sdsm_plan_mask_bytes(const sdsm_plan *p) { return p ? (size_t)std::max<int64_t>(p->total_mask_words, 1) * 4 : 0; }
extern "C" int64_t sdsm_plan_total_pixels(const sdsm_plan *p) { return p ? p->total_pixels : 0; }
extern "C" int64_t sdsm_plan_xi_count(const sdsm_plan *p) { return p ? std::max<int64_t>(p->total_xi, 1) : 0; }

extern "C" int sdsm_plan_describe(const sdsm_plan *p, int32_t *mask_info, int64_t *mask_offset, int32_t *n_pixels)
{
    if (!p) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_describe: null plan");
    if (mask_info) memcpy(mask_info, p->mask_info.data(), p->mask_info.size() * 4);
    if (mask_offset) memcpy(mask_offset, p->mask_off_bytes.data(), p->mask_off_bytes.size() * 8);
    if (n_pixels) memcpy(n_pixels, p->n_pixels.data(), p->n_pixels.size() * 4);
    return SDSM_OK;
}

extern "C" int sdsm_plan_schedule(const sdsm_plan *p, int32_t *group_members, int32_t *rows_workgroups)
{
    if (!p) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_schedule: null plan");
    for (int i = 0; i < p->n; i++) {
        if (group_members) group_members[i] = p->cand[i].wide_g;
        if (rows_workgroups) rows_workgroups[i] = p->cand[i].rows_g;
    }
    return SDSM_OK;
}

// The launch lists of the plan in its current mode: spans = (first, count) in `order` of [all | beyond class 1 | beyond class 2 | group members |
// row members | setup small | setup big]; order (if given): the entries of all lists, as many as the counts add up to.
extern "C" int sdsm_plan_lists(const sdsm_plan *p, int32_t spans[14], int32_t *order)
{
    if (!p || !spans) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_lists: null argument");
    memcpy(spans, &p->lists, sizeof(LaunchLists));
    if (order) memcpy(order, p->order.data(), p->order.size() * 4);
    return SDSM_OK;
}

// The solve class (SDSM_CLS_* of sdsm_solve_class: 0 class 1, 1 class 1b, 2 class 2, 3 class 2b, 4 global memory, 5 / 6 / 7 groups of class-2 / class-2b / light
// layout, -1 none) of every candidate of the plan in its current mode, given what the setup kernel found (status, M and env_size of its CandState).
extern "C" int sdsm_plan_solve_classes(const sdsm_plan *p, const int32_t *status, const int32_t *M, const int32_t *env_size, int32_t *cls)
{
    if (!p || !status || !M || !env_size || !cls) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_solve_classes: null argument");
    const int light = light_limit(p);
    for (int i = 0; i < p->n; i++) cls[i] = sdsm_solve_class(status[i], M[i], env_size[i], p->cand[i].N, p->cand[i].wide_g, p->wide_pixels, light);
    return SDSM_OK;
}

extern "C" int sdsm_plan_xi_offsets(const sdsm_plan *p, int64_t *xi_offset)
{
    if (!p || !xi_offset) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_xi_offsets: null argument");
    memcpy(xi_offset, p->xi_off.data(), p->xi_off.size() * 8);
    return SDSM_OK;
}

extern "C" int sdsm_plan_layout(const sdsm_plan *p, int64_t *out)
{
    if (!p || !out) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_layout: null argument");
    int64_t v[16] = {(int64_t)p->off_cand, (int64_t)p->off_state, (int64_t)p->off_crop_y, (int64_t)p->off_crop_rc, (int64_t)p->off_crop_cc,
                     (int64_t)p->off_run_meta, (int64_t)p->off_grid, (int64_t)p->off_ell_im, (int64_t)p->off_ell_w, p->zcap_run, p->k,
                     (int64_t)sizeof(CandDesc), p->total_pixels, p->total_ell, (int64_t)sizeof(CandState), p->total_runs};
    memcpy(out, v, sizeof(v));
    return SDSM_OK;
}

extern "C" int sdsm_batch_upload(const sdsm_plan *p, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!p || !d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_upload: null argument");
    if (ws_bytes < p->total) return fail(SDSM_ERR_WORKSPACE, "sdsm_batch_upload: workspace too small");
    if (p->n == 0) { p->uploaded_gen = p->layout_gen; p->uploaded_ws = d_ws; return SDSM_OK; }
    uint8_t *b = (uint8_t *)d_ws;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemcpyAsync(b + p->off_cand, p->cand.data(), sizeof(CandDesc) * p->n, hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload cand");
    if (!p->fp_labels.empty() && (e = hipMemcpyAsync(b + p->off_fp, p->fp_labels.data(), 4 * p->fp_labels.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload footprints");
    if ((e = hipMemcpyAsync(b + p->off_order, p->order.data(), 4 * p->order.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload order");
    if ((e = hipMemcpyAsync(b + p->off_psf, p->psf.data(), 4 * p->psf.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hipfail(e, "upload psf");
    if ((e = hipMemsetAsync(b + p->off_words, 0, sizeof(LaunchWords), s)) != hipSuccess) return hipfail(e, "hipMemsetAsync");   // (the event counters read 0 before the first launch)
    p->uploaded_gen = p->layout_gen; p->uploaded_ws = d_ws;
    return SDSM_OK;
}

static thread_local long long *g_prof = nullptr;
// Time a member of a workgroup group waits for its partners at one exchange before the group is given up (the candidate is then solved again
// without a group: correct, one more launch).  50 ms: a partner that is not resident by then is waiting for a compute unit behind other work --
// several processes sharing the card --, and the retry costs less than the wait (round 3 waited 10 s).
#define SDSM_GROUP_TIMEOUT_TICKS 5000000ll
static thread_local long long g_wide_timeout = SDSM_GROUP_TIMEOUT_TICKS;   // ticks of the 100 MHz wall clock
extern "C" int sdsm_set_group_timeout_us(double us) { g_wide_timeout = us > 0 ? (long long)(us * 100.0) : SDSM_GROUP_TIMEOUT_TICKS; return SDSM_OK; }

// Whether the caller's stream and the side streams of the last launch of this process that needed them run side by side: 1 yes, 0 fewer than three
// side streams with a hardware queue of their own could be found (classes of a launch then run one after the other: correct, slower), -1 not known (no
// launch needed side streams so far, or the probe stayed undecided).
static std::atomic<int> g_queues_distinct{-1};
static std::atomic<int> g_side_report[8];
extern "C" int sdsm_side_queues_distinct(void) { return g_queues_distinct.load(std::memory_order_relaxed); }
extern "C" int sdsm_side_queue_report(int32_t out[8])
{
    if (!out) return fail(SDSM_ERR_ARGUMENT, "sdsm_side_queue_report: null argument");
    for (int i = 0; i < 8; i++) out[i] = g_side_report[i].load(std::memory_order_relaxed);
    return SDSM_OK;
}
extern "C" hipError_t sdsm_launch_queue_probe(int32_t *d_words, const hipStream_t *streams, int n);
extern "C" int sdsm_solve_wants_own_2b(int n_w, int n_d);

// The choice of side streams as a function of a given "shares a hardware queue" relation: shares is (n_pool + 1)^2, index 0 the caller's stream, index
// 1 + i pool stream i; an entry set in either direction counts.  Greedy: S = {caller}; pool streams in the order of their creation; a stream joins S if
// it shares with no member of S; until `want` have joined.  out[0 .. want-1]: pool indices of side 1, 2, ...; returns how many are clean.  Missing
// sides are replaced: side 3 (class 1b) goes behind side 2 (the groups / class 2), then side 2 behind side 1 -- the two group kernels end the launch and get
// the clean queues first; a side beyond the third (class 2b of plans without groups) is simply absent (-1).  Nothing clean: pool stream 0 for all
// (every class behind the caller's own kernels: still correct); an empty pool: all -1.
extern "C" int sdsm_choose_sides_host(int n_pool, const uint8_t *shares, int want, int32_t *out)
{
    if (n_pool < 0 || want < 0 || !out || (n_pool > 0 && !shares)) return -1;
    const int n = n_pool + 1;
    std::vector<int> S{0};
    int clean = 0;
    for (int c = 1; c < n && clean < want; c++) {
        bool ok = true;
        for (int m : S) if (shares[c * n + m] || shares[m * n + c]) { ok = false; break; }
        if (ok) { S.push_back(c); out[clean++] = c - 1; }
    }
    for (int i = clean; i < want; i++) out[i] = i >= 3 ? -1 : i > 0 ? out[i - 1] : n_pool > 0 ? 0 : -1;
    return clean;
}

static bool grow_pool(SideSet *q, int upto)
{
    // Default priority.  (High priority for these queues -- the few long candidates of a launch are on them -- changes nothing where the
    // launch is short and costs 3 ms of the 71 of the synthetic 4096^2 launch, where every class has work: measured, round 3.  A fourth
    // side stream for class 2, beside the groups instead of behind them: 8 different BBBC039-like images 8.2 -> 8.5 ms, GOWT1-like
    // 4.9 -> 5.2: its 256 resident workgroups take compute units from the group members at the start.)
    while (q->n_pool < upto && q->n_pool < SDSM_SIDE_POOL) {
        if (hipStreamCreateWithFlags(&q->pool[q->n_pool], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return false; }
        q->n_pool++;
    }
    return q->n_pool >= upto;
}

// One probe of n streams, the candidate last (sdsm_k_queue_probe, <= 2 ms), all of them idle when it starts.  1: they ran side by side.  A probe that
// timed out is repeated (a busy chip times out too) up to `attempts` times; 0: in two probes the candidate started only when the same member had ended (or
// the other way round): it shares a hardware queue with a member -- *partner is the first such position in st; the members all give up at about the same time, so
// it need not be THE one --; -1: timed out, no such evidence (or a HIP call failed): undecided.
static int probe_set(SideSet *q, const hipStream_t *st, int n, int attempts, int *partner)
{
    struct { int32_t arrived, timed_out, pad[2]; long long stamp[2 * SDSM_PROBE_MAX]; } res;
    static_assert(sizeof(res) == SDSM_PROBE_BYTES, "layout of the probe words");
    uint32_t serial_before = 0;
    for (int a = 0; a < attempts; a++) {
        bool ok = true;
        for (int i = 0; i < n; i++) ok = hipStreamSynchronize(st[i]) == hipSuccess && ok;
        ok = ok && hipMemsetAsync(q->probe_words, 0, SDSM_PROBE_BYTES, st[0]) == hipSuccess && hipStreamSynchronize(st[0]) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); return -1; }
        q->probes++;
        ok = sdsm_launch_queue_probe(q->probe_words, st, n) == hipSuccess;
        for (int i = 0; i < n; i++) ok = hipStreamSynchronize(st[i]) == hipSuccess && ok;      // (also after a failed launch: whatever was queued has run)
        ok = ok && hipMemcpy(&res, q->probe_words, SDSM_PROBE_BYTES, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); return -1; }
        if (res.arrived == n && !res.timed_out) return 1;
        uint32_t serial = 0;
        const int c = n - 1;
        for (int i = 0; i < c; i++) if (res.stamp[2 * c] >= res.stamp[2 * i + 1] || res.stamp[2 * i] >= res.stamp[2 * c + 1]) serial |= 1u << i;
        if (a > 0 && (serial & serial_before)) { *partner = __builtin_ctz(serial & serial_before); return 0; }
        serial_before = serial;
    }
    return -1;
}

// The side streams for launches from `caller` (under the set's mutex): from the cache, or -- once per caller stream, before any of the launch's work
// is queued -- found by probing: the caller's stream with the first three pool streams at once (the common case: one probe), else pool stream by pool
// stream (sdsm_choose_sides_host's greedy rule with the probe as its oracle).  This synchronises the caller's stream and the pool.
static hipError_t choose_sides(SideSet *q, hipStream_t caller, int want, SideChoice *out)
{
    SideChoice *hit = nullptr;
    for (SideChoice &c : q->cache) if (c.valid && c.caller == caller) hit = &c;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (caller && hipStreamIsCapturing(caller, &capture) != hipSuccess) { (void)hipGetLastError(); capture = hipStreamCaptureStatusNone; }
    const bool capturing = capture != hipStreamCaptureStatusNone;       // (a capturing stream cannot be synchronised: no probe, and nothing is remembered)
    if (hit && (capturing || (hit->want >= want && (hit->state != -1 || hit->reprobes >= 3)))) { *out = *hit; }
    else {
        SideChoice c;
        c.caller = caller; c.want = want; c.reprobes = hit ? hit->reprobes + (hit->state == -1 ? 1 : 0) : 0;
        if (!grow_pool(q, 1)) return hipErrorOutOfMemory;
        uint8_t found[(SDSM_SIDE_POOL + 1) * (SDSM_SIDE_POOL + 1)] = {0};   // "shares a queue" as the probes find it, row / column 0 the caller's stream
        bool unknown = capturing;
        if (!capturing && !q->probe_words && hipMalloc((void **)&q->probe_words, SDSM_PROBE_BYTES) != hipSuccess) { q->probe_words = nullptr; (void)hipGetLastError(); unknown = true; }
        if (unknown) grow_pool(q, want);
        else {
            hipStream_t st[SDSM_PROBE_MAX];
            int chosen[4], n_chosen = 0, next = 0, partner = 0;
            st[0] = caller;
            if (grow_pool(q, 3)) {
                for (int i = 0; i < 3; i++) st[1 + i] = q->pool[i];
                if (probe_set(q, st, 4, 1, &partner) == 1) { for (int i = 0; i < 3; i++) chosen[i] = i; n_chosen = next = 3; }
            }
            while (n_chosen < want && next < SDSM_SIDE_POOL && grow_pool(q, next + 1)) {
                for (int i = 0; i < n_chosen; i++) st[1 + i] = q->pool[chosen[i]];
                st[1 + n_chosen] = q->pool[next];
                const int r = probe_set(q, st, n_chosen + 2, 2, &partner);
                if (r == 0) found[(next + 1) * (SDSM_SIDE_POOL + 1) + (partner == 0 ? 0 : chosen[partner - 1] + 1)] = 1;
                else {
                    if (r < 0) { unknown = true; q->unknowns++; }    // undecided: the candidate is used, and the caller stream is probed again at a later launch
                    chosen[n_chosen++] = next;
                }
                next++;
            }
        }
        const int n = q->n_pool + 1;                                   // (the pool grew while `found` was filled in: the relation at its final size)
        uint8_t shares[(SDSM_SIDE_POOL + 1) * (SDSM_SIDE_POOL + 1)] = {0};
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) shares[i * n + j] = found[i * (SDSM_SIDE_POOL + 1) + j];
        int32_t idx[4] = {-1, -1, -1, -1};
        c.clean = sdsm_choose_sides_host(q->n_pool, shares, want, idx);
        for (int i = 0; i < 4; i++) c.idx[i] = idx[i];
        c.state = c.clean < 3 ? 0 : unknown ? -1 : 1;
        c.born = ++q->tick; c.valid = true;
        if (!capturing) {
            SideChoice *slot = hit;
            if (!slot) { slot = &q->cache[0]; for (SideChoice &o : q->cache) { if (!o.valid) { slot = &o; break; } if (o.born < slot->born) slot = &o; } }
            *slot = c;
        }
        if (c.state == 0 && !q->warned) {
            q->warned = true;
            const char *v = getenv("GPU_MAX_HW_QUEUES");
            fprintf(stderr, "superdsm_amd: only %d of the 3 side streams of a launch found a hardware queue of their own among %d streams (GPU_MAX_HW_QUEUES=%s): solve classes "
                            "of a launch run one after the other -- correct, slower.  A launch needs 4 hardware queues (HIP's default); other streams of the process in use at "
                            "the same time take queues away.\n", c.clean, q->n_pool, v ? v : "unset: 4");
        }
        *out = c;
    }
    g_queues_distinct.store(out->state == 1 ? 1 : out->state == 0 ? 0 : -1, std::memory_order_relaxed);
    const int rep[8] = {q->n_pool, out->clean, q->probes, out->idx[0], out->idx[1], out->idx[2], out->idx[3], q->unknowns};
    for (int i = 0; i < 8; i++) g_side_report[i].store(rep[i], std::memory_order_relaxed);
    return hipSuccess;
}
// Diagnostic builds (-DSDSM_PROFILE): device buffer of 8 int64 cycle counters per candidate, see DESIGN.md.
extern "C" int sdsm_set_debug_buffer(void *d_buf) { g_prof = (long long *)d_buf; return SDSM_OK; }


#ifndef SDSM_HESS_THR
#define SDSM_HESS_THR 0.1f    // same constant as the oracle's ORC_HESS_THR
#endif
static std::atomic<int> g_solver_diag{0};      // sdsm_set_solver_diagnostics (process-wide)
// Kernel arguments of a plan laid out in the caller's workspace.
static BatchParams make_params(const sdsm_plan *p, void *d_ws)
{
    uint8_t *b = (uint8_t *)d_ws;
    BatchParams P{};
    P.n = p->n; P.n_total = p->n; P.latency = p->mode == 1; P.n_images = (int)p->images.size();
    for (size_t i = 0; i < p->images.size(); i++) { P.img[i].H = p->images[i].H; P.img[i].W = p->images[i].W; }   // device pointers: filled by the launch
    P.k = p->k; P.R = p->R; P.subsample = p->cfg.smooth_subsample; P.zcap = p->zcap; P.zcap_run = p->zcap_run; P.zshift = p->zshift; P.no_deform = p->no_deform; P.no_trivial_rule = p->cfg.flags & 1;
    P.init_elliptical = p->cfg.init_elliptical; P.max_iters = p->cfg.max_iters; P.k1_pixmax = p->wide_pixels; P.boost_pixels = p->boost_pixels; P.rows_mcap = p->rows_mcap; P.solver_diag = g_solver_diag.load(std::memory_order_relaxed);
    P.light_emax = light_limit(p); P.wide_rest = p->wide_rest;
    P.scale = p->cfg.scale; P.epsilon = p->cfg.epsilon; P.alpha = p->cfg.alpha; P.reg_unit = p->cfg.alpha * std::sqrt(p->cfg.epsilon);
    P.cand = (const CandDesc *)(b + p->off_cand); P.state = (CandState *)(b + p->off_state);
    P.fp_labels = (const int32_t *)(b + p->off_fp); P.order = (const int32_t *)(b + p->off_order);
    P.crop_y = (double *)(b + p->off_crop_y); P.crop_rc = (uint32_t *)(b + p->off_crop_rc); P.crop_cc = (uint32_t *)(b + p->off_crop_cc);
    P.dist = (uint32_t *)(b + p->off_dist); P.grid_rc = (uint32_t *)(b + p->off_grid);
    P.ell_im = (uint32_t *)(b + p->off_ell_im); P.ell_w = (float *)(b + p->off_ell_w); P.run_meta = (uint32_t *)(b + p->off_run_meta);
    P.run_q0 = (uint32_t *)(b + p->off_run_q0); P.run_aux = (uint32_t *)(b + p->off_run_aux);
    P.tmp_y = (double *)(b + p->off_tmp_y); P.tmp_rc = (uint32_t *)(b + p->off_tmp_rc); P.inv = (uint32_t *)(b + p->off_inv);
    P.hess_thr = SDSM_HESS_THR;
    P.psf = (const float *)(b + p->off_psf);
    P.env_fst = (int32_t *)(b + p->off_env_fst); P.env_rb = (int32_t *)(b + p->off_env_rb);
    P.hglob = (double *)(b + p->off_hglob); P.wide_pool = (double *)(b + p->off_wide);
    P.wide_ticket = (int32_t *)(b + p->off_words + offsetof(LaunchWords, ticket)); P.wide_timeout = g_wide_timeout;
    P.cls_count = (int32_t *)(b + p->off_words + offsetof(LaunchWords, list_head));
    P.prof = g_prof; P.prof2 = g_prof ? g_prof + (size_t)16 * p->n : nullptr;
    P.x0 = p->x0;
    return P;
}

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

extern "C" int sdsm_set_solver_diagnostics(int flags)
{
    if (flags & ~1) return fail(SDSM_ERR_ARGUMENT, "sdsm_set_solver_diagnostics: unknown flag bit (1: recompute at unchanged iterates)");
    g_solver_diag.store(flags, std::memory_order_relaxed);
    return SDSM_OK;
}

// Diagnostic: the envelope limit of the light group class for the launches that follow, in every plan with groups (tests move a small region across it); negative: the default (light_limit).
extern "C" int sdsm_set_light_envelope_limit(int doubles)
{
    if (doubles > SDSM_KL_EMAX) return fail(SDSM_ERR_ARGUMENT, "sdsm_set_light_envelope_limit: at most SDSM_KL_EMAX (12400) doubles fit the light layout");
    g_light_emax.store(doubles < 0 ? -1 : doubles, std::memory_order_relaxed);
    return SDSM_OK;
}

extern "C" int sdsm_batch_solver_counters(const sdsm_plan *p, void *d_ws, int64_t out[4])
{
    if (!p || !d_ws || !out) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_solver_counters: null argument");
    if (p->uploaded_ws != d_ws) return fail(SDSM_ERR_ARGUMENT, "sdsm_batch_solver_counters: not the workspace of the plan's upload (sdsm_batch_upload)");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (p->n == 0) return SDSM_OK;
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hipfail(e, "hipDeviceSynchronize");
    if ((e = hipMemcpy(out, (const uint8_t *)d_ws + p->off_words + offsetof(LaunchWords, counters), sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess) return hipfail(e, "hipMemcpy");
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
    if ((e = hipMemsetAsync((uint8_t *)d_ws + p->off_words, 0, sizeof(LaunchWords), s)) != hipSuccess) return hipfail(e, "hipMemsetAsync");   // tickets, list heads, counters
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
    if ((e = hipMemcpyAsync(st.data(), (const uint8_t *)d_ws + p->off_state, sizeof(CandState) * p->n, hipMemcpyDeviceToHost, s)) != hipSuccess) return hipfail(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hipfail(e, "hipStreamSynchronize");
    for (int i = 0; i < p->n; i++) n_deform[i] = st[i].status == ST_OK ? (6 + st[i].M > SDSM_MAX_N_GLOBAL ? 0 : st[i].M) : -1;   // (beyond the solver's limit: elliptical model only)
    return SDSM_OK;
}

// Starting points of the DSM solves of the following launches of this plan: d_x0 holds sdsm_plan_eval_param_count() doubles in the layout of
// sdsm_batch_eval's d_params (candidate i: theta[6] in full-image-normalised coordinates, then xi[M], at 6 i + xi_offset[i]) and must stay
// valid until those launches have completed; null = none.  Only plans created with init_elliptical = 0 read it; a fallback
// (SDSM_CAND_FALLBACK) then returns this initialisation, as the reference does (objects.py:409-410).
extern "C" int sdsm_plan_set_start(const sdsm_plan *p, const double *d_x0)
{
    if (!p) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_set_start: null plan");
    if (d_x0 && p->cfg.init_elliptical) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_set_start: the plan solves the elliptical model first (init_elliptical = 1)");
    p->x0 = d_x0;
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

extern "C" int64_t sdsm_plan_eval_param_count(const sdsm_plan *p) { return p ? (int64_t)6 * p->n + std::max<int64_t>(p->total_xi, 1) : 0; }
extern "C" int64_t sdsm_plan_eval_out_count(const sdsm_plan *p) { return p ? (int64_t)29 * p->n + std::max<int64_t>(p->total_xi, 1) : 0; }

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

extern "C" int sdsm_measure_objects_multi(const sdsm_set_image *images, int n_images, int n, const int32_t *d_obj_image, const int32_t *d_boxes,
                                          const int64_t *d_bits_off, const uint32_t *d_bits, const double *d_g, double *d_gmax_abs,
                                          int32_t *d_scale_exp, sdsm_measure_record *d_out, void *stream)
{
    SET_TABLE("sdsm_measure_objects", SET_SIDES | SET_PIXELS);
    if (n < 0) return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_objects: n < 0");
    if (d_g && !d_gmax_abs) return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_objects: intensities need d_gmax_abs");
    if (n > 0 && (!d_boxes || !d_bits_off || !d_bits || !d_out || (n_images > 1 && !d_obj_image)))
        return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_objects: null argument");
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
    for (int i = 0; i < n_images; i++) {
        if (n_labels[i] < 1 || n_labels[i] > SDSM_MEASURE_MAX_LABELS || rec_off[i] < 0)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_labels: 1 <= n_labels <= 65536 and rec_off >= 0 required");
        for (int j = 0; j < i; j++)
            if (rec_off[i] < rec_off[j] + n_labels[j] && rec_off[j] < rec_off[i] + n_labels[i])
                return fail(SDSM_ERR_ARGUMENT, "sdsm_measure_labels: the records of two images overlap");
    }
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

// ---- contingency table of two label maps (sdsm_measure.hip) ---------------------------------------------------------------------------
extern "C" hipError_t sdsm_overlap_pairs_impl(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b,
                                              const int64_t *table_off, const int64_t *capacity, uint64_t *d_keys, uint64_t *d_counts,
                                              int32_t *d_status, hipStream_t stream);

extern "C" int sdsm_overlap_pairs_multi(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b, const int64_t *table_off,
                                        const int64_t *capacity, uint64_t *d_keys, uint64_t *d_counts, int32_t *d_status, void *stream)
{
    SET_TABLE("sdsm_overlap_pairs", SET_PIXELS);
    if (!d_a || !d_b || !table_off || !capacity || !d_keys || !d_counts || !d_status) return fail(SDSM_ERR_ARGUMENT, "sdsm_overlap_pairs: null argument");
    for (int i = 0; i < n_images; i++) {
        if (capacity[i] < 1 || (capacity[i] & (capacity[i] - 1)) != 0 || table_off[i] < 0)
            return fail(SDSM_ERR_ARGUMENT, "sdsm_overlap_pairs: capacity a power of two >= 1 and table_off >= 0 required");
        for (int j = 0; j < i; j++)
            if (table_off[i] < table_off[j] + capacity[j] && table_off[j] < table_off[i] + capacity[i])
                return fail(SDSM_ERR_ARGUMENT, "sdsm_overlap_pairs: the tables of two images overlap");
    }
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

// H^2 + W^2 < 2^31: every squared distance fits int32 (and so every side 16 bits, H * W 30 bits)
static bool boundary_shapes_ok(const sdsm_set_image *images, int n_images)
{
    for (int i = 0; i < n_images; i++)
        if ((int64_t)images[i].H * images[i].H + (int64_t)images[i].W * images[i].W >= (int64_t)1 << 31) return false;
    return true;
}
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
