// The plan of a batch: what sdsm_plan_create(_multi) derives from the caller's footprints and atom statistics -- per-candidate descriptors, the
// PSF, workgroup groups, launch lists, the workspace layout (the table of sdsm_plan.h) -- every sdsm_plan_* query, and the kernel arguments of a
// plan in a workspace (make_params) with the process-wide diagnostic settings that enter them.  Also the error text of include/sdsm.h.  Pure host
// arithmetic: no HIP runtime call, no symbol of another translation unit, so the unit links alone and runs under sanitizers on a machine
// without a GPU (tests/host/plan_check.cpp).
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "sdsm_plan.h"

static thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }

extern "C" int sdsm_version(void) { return SDSM_VERSION; }
extern "C" const char *sdsm_last_error(void) { return g_err.c_str(); }

// ---- the weights of a Gaussian filter on the host (the PSF below; sdsm_prepare.hip's filters declare and call it) ----------------------
// numpy pairwise sum (PW_BLOCKSIZE 128), host
static double np_pairwise(const double *a, long n)
{
    if (n < 8) { double r = 0; for (long i = 0; i < n; i++) r += a[i]; return r; }
    if (n <= 128) {
        double r[8]; long i;
        for (int k = 0; k < 8; k++) r[k] = a[k];
        for (i = 8; i < n - (n % 8); i += 8) for (int k = 0; k < 8; k++) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    long n2 = n / 2; n2 -= n2 % 8;
    return np_pairwise(a, n2) + np_pairwise(a + n2, n - n2);
}

// scipy.ndimage._filters._gaussian_kernel1d
extern "C" void sdsm_gauss_kernel_host(double sigma, int radius, double *w)
{
    double s2 = sigma * sigma;
    for (int i = 0; i <= 2 * radius; i++) { double x = i - radius; w[i] = exp(-0.5 / s2 * (x * x)); }
    double s = np_pairwise(w, 2 * radius + 1);
    for (int i = 0; i <= 2 * radius; i++) w[i] = w[i] / s;
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

// ---- plan ------------------------------------------------------------------------------------------------
static std::atomic<int> g_light_emax{-1};   // sdsm_set_light_envelope_limit (process-wide): -1 = the rule of light_limit()

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
static int light_limit(const sdsm_plan *p)
{
    if (!SDSM_LIGHT_GROUPS || p->lists.group_members.count <= 0) return 0;
    const int v = g_light_emax.load(std::memory_order_relaxed);
    if (v >= 0) return v;
    return p->n > SDSM_LIGHT_MIN_CANDIDATES ? SDSM_KL_EMAX : 0;
}

// The diagnostic environment knobs of a layout (unsupported), read at every layout.
struct LayoutKnobs { long long tp_min = SDSM_WIDE_TP_MIN_PIXELS, k1_pixdiv = SDSM_K1_PIXDIV; long wide_slice = SDSM_WIDE_SLICE; };
static LayoutKnobs read_knobs()
{
    LayoutKnobs k;
    if (const char *e = getenv("SDSM_WIDE_TP_MIN_PIXELS")) { const long long v = atoll(e); if (v > 0) k.tp_min = v; }
    if (const char *e = getenv("SDSM_K1_PIXDIV")) { const long long v = atoll(e); if (v > 0) k.k1_pixdiv = v; else if (v < 0) k.k1_pixdiv = 0; }   // (negative: no bound)
    if (const char *e = getenv("SDSM_WIDE_SLICE")) { const long v = atol(e); if (v > 0) k.wide_slice = v; }
    return k;
}

// Which regions get a workgroup group, and of how many members, before the member budget.
struct GroupRule {
    bool groups, latency; int n; long long wide_thr; long wide_slice;     // wide_thr: regions with more pixels get a group of one member per wide_slice pixels
    long size(long N) const      // members of the group a region of N pixels would get (0: none)
    {
        if (!groups || n >= (1 << 24)) return 0;
        if (N > wide_thr) return std::min<long>(SDSM_WIDE_MAX_G, std::max<long>(2, (N + wide_slice - 1) / wide_slice));
        if (latency && N > SDSM_WIDE_PIXELS) return std::min<long>(SDSM_LAT_GMAX, std::max<long>(2, (N + SDSM_LAT_SLICE - 1) / SDSM_LAT_SLICE));   // latency mode: the largest regions of an ordinary image too
        return 0;
    }
};

// Step 1, thresholds: the pixel bounds of the mode (wide_pixels, boost_pixels) and the rule of the groups.
// Groups shorten the longest chains of a launch; every member holds a whole compute unit and a group only advances while all of its
// members are resident.  In throughput mode the LARGEST regions get groups until their members add up to the compute units of the
// chip; very large regions beyond that (synthetic 4096^2 image: 434 of them, 1296 members -- they waited for each other behind the
// small classes) are solved as ordinary class-2 candidates, one workgroup each.
static GroupRule layout_thresholds(sdsm_plan *p, const LayoutKnobs &knobs)
{
    const bool latency = p->mode == 1, groups = p->mode != 2;
    long long all_pixels = 0;
    for (const CandDesc &c : p->cand) all_pixels += c.N;
    p->wide_pixels = latency ? SDSM_WIDE_PIXELS : INT_MAX;
    // Throughput mode: a candidate whose chain (~ its pixels) is long next to the time the plan keeps the chip busy (~ pixels of all
    // candidates / 1024 workgroup slots of class 1) runs its passes over the pixels at a raised issue priority: regions above 1 /
    // SDSM_K1_PIXDIV of all pixels.  8 different BBBC039-like images: class 1 took 6.8 ms beside the other classes while its workgroup
    // time was 3.6 ms of the chip -- its 4-5 ms chains (6-7 k pixels, 95-114 unknowns; 2.8 ms on an idle chip) ended it.  (Moving
    // them to the 512-thread classes instead, a compute unit each: 7.6 -> 8.7-9.2 ms per step, measured in round 4.)
    p->boost_pixels = !latency && knobs.k1_pixdiv > 0 ? (int)std::min<long long>(INT_MAX, std::max<long long>(SDSM_WIDE_PIXELS, all_pixels / knobs.k1_pixdiv)) : INT_MAX;
    // Throughput mode groups only regions whose chain (~ its pixels) is long next to the time the whole plan keeps the chip busy (~ all pixels / compute units):
    // the synthetic 4096^2 plan (10 073 candidates, 50 M pixels) gets no groups at all -- its 31 k-pixel regions end long before the rest does,
    // and groups there cost compute units that the other candidates wait for (75 -> 97 ms with groups for everything above 12 288 pixels)
    const long long wide_thr = groups && !latency ? std::max<long long>(knobs.tp_min, all_pixels / SDSM_WIDE_FILL) : SDSM_WIDE_MIN_PIXELS;
    return GroupRule{groups, latency, p->n, wide_thr, knobs.wide_slice};
}

// Step 2, groups: the members of every candidate's group (0: none) within the member budget -- both modes: a single image with many large
// clusters (636 candidates, 16 k-pixel regions) asked for several hundred members in latency mode and took 15 ms instead of 12 --, the
// largest regions first, and the bonus members inside the same budget.
static std::vector<long> layout_groups(const sdsm_plan *p, const GroupRule &rule)
{
    const int n = p->n;
    std::vector<long> G(n, 0);
    std::vector<int> big;
    for (int i = 0; i < n; i++) if (rule.size(p->cand[i].N) > 0) big.push_back(i);
    std::stable_sort(big.begin(), big.end(), [&](int a, int b) { return p->cand[a].N > p->cand[b].N; });
    long members = 0;
    int cutoff = 0;                                  // regions of at most this many pixels get no group (equal regions are treated alike)
    for (int i : big) {
        members += rule.size(p->cand[i].N);
        if (members > SDSM_WIDE_MAX_MEMBERS) { cutoff = p->cand[i].N; break; }
    }
    long used = 0, nmax = 0;
    for (int i : big) if (p->cand[i].N > cutoff) { G[i] = rule.size(p->cand[i].N); used += G[i]; nmax = std::max<long>(nmax, p->cand[i].N); }
    if (SDSM_WIDE_BONUS > 0 && rule.groups && !rule.latency) {
        for (int i : big) {
            if (G[i] == 0 || 6 + (long)p->cand[i].Mcap <= SDSM_KL_NMAX || (long long)p->cand[i].N * 100 < (long long)nmax * SDSM_WIDE_BONUS_PCT) continue;
            const long b = std::min<long>(std::min<long>(SDSM_WIDE_BONUS, SDSM_WIDE_MAX_G - G[i]), SDSM_WIDE_MAX_MEMBERS - used);
            if (b > 0) { G[i] += b; used += b; }
        }
    }
    return G;
}

// Step 3, members: per candidate the group members, the workgroups that build its rows of G~, and its block of the wide pool.
static void layout_members(sdsm_plan *p, const std::vector<long> &groups)
{
    const int n = p->n;
    long rows_regions = 0;
    for (int i = 0; i < n; i++) rows_regions += p->cand[i].N > SDSM_ROWS_MIN_PIXELS;
    const bool rows_multi = rows_regions <= SDSM_ROWS_MAX_REGIONS;
    p->n_wide = 0;
    p->wide_rest = 0;
    for (int i = 0; i < n; i++) {
        CandDesc &c = p->cand[i];
        const long G = groups[i];
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
        if (G > 0 && 6 + (long)c.Mcap > SDSM_K2B_NMAX) p->wide_rest = 1;
    }
}

// Step 4, lists: the one place that lays the launch lists out in `order`.
static void layout_lists(sdsm_plan *p)
{
    const int n = p->n;
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
    // (the initialisers run left to right)
    p->order.clear();
    auto put = [&](const std::vector<int32_t> &list) { const ListSpan at{(int32_t)p->order.size(), (int32_t)list.size()}; p->order.insert(p->order.end(), list.begin(), list.end()); return at; };
    p->lists = LaunchLists{put(all), put(beyond_1), put(beyond_2), put(group_members), put(row_members), put(setup_small), put(setup_big)};
}

// Step 5, workspace: the offsets of the blocks of the table (sdsm_plan.h), the launch words behind them, and the size.
static void layout_workspace(sdsm_plan *p)
{
    size_t o = 0;
#define X(name, T, count) p->ws_off[WS_##name] = o; o += al(sizeof(T) * (size_t)(count));
    SDSM_WS_BLOCKS(X)
#undef X
    p->ws_off[WS_words] = o;
    p->total = o + al(sizeof(LaunchWords));
}

// Workgroup groups, launch lists and workspace layout (repeated when the scheduling mode changes).
static void layout_plan(sdsm_plan *p)
{
    const LayoutKnobs knobs = read_knobs();
    p->layout_gen++;
    layout_members(p, layout_groups(p, layout_thresholds(p, knobs)));
    layout_lists(p);
    layout_workspace(p);
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

// A query's array to the caller, if asked for (an empty plan has nothing to copy, and no address to copy from).
template <class T> static void copy_out(void *out, const std::vector<T> &v) { if (out && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(T)); }

extern "C" int sdsm_plan_describe(const sdsm_plan *p, int32_t *mask_info, int64_t *mask_offset, int32_t *n_pixels)
{
    if (!p) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_describe: null plan");
    copy_out(mask_info, p->mask_info); copy_out(mask_offset, p->mask_off_bytes); copy_out(n_pixels, p->n_pixels);
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
    copy_out(order, p->order);
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
    copy_out(xi_offset, p->xi_off);
    return SDSM_OK;
}

extern "C" int sdsm_plan_layout(const sdsm_plan *p, int64_t *out)
{
    if (!p || !out) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_layout: null argument");
    const int64_t v[16] = {(int64_t)p->ws_off[WS_cand], (int64_t)p->ws_off[WS_state], (int64_t)p->ws_off[WS_crop_y], (int64_t)p->ws_off[WS_crop_rc], (int64_t)p->ws_off[WS_crop_cc],
                           (int64_t)p->ws_off[WS_run_meta], (int64_t)p->ws_off[WS_grid_rc], (int64_t)p->ws_off[WS_ell_im], (int64_t)p->ws_off[WS_ell_w], p->zcap_run, p->k,
                           (int64_t)sizeof(CandDesc), p->total_pixels, p->total_ell, (int64_t)sizeof(CandState), p->total_runs};
    memcpy(out, v, sizeof(v));
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

extern "C" int64_t sdsm_plan_eval_param_count(const sdsm_plan *p) { return p ? (int64_t)6 * p->n + std::max<int64_t>(p->total_xi, 1) : 0; }
extern "C" int64_t sdsm_plan_eval_out_count(const sdsm_plan *p) { return p ? (int64_t)29 * p->n + std::max<int64_t>(p->total_xi, 1) : 0; }

// ---- the kernel arguments of a plan, and the process-wide diagnostic settings that enter them --------------------------------------------
static thread_local long long *g_prof = nullptr;
// Time a member of a workgroup group waits for its partners at one exchange before the group is given up (the candidate is then solved again
// without a group: correct, one more launch).  50 ms: a partner that is not resident by then is waiting for a compute unit behind other work --
// several processes sharing the card --, and the retry costs less than the wait (round 3 waited 10 s).
#define SDSM_GROUP_TIMEOUT_TICKS 5000000ll
static thread_local long long g_wide_timeout = SDSM_GROUP_TIMEOUT_TICKS;   // ticks of the 100 MHz wall clock
extern "C" int sdsm_set_group_timeout_us(double us) { g_wide_timeout = us > 0 ? (long long)(us * 100.0) : SDSM_GROUP_TIMEOUT_TICKS; return SDSM_OK; }
// Diagnostic builds (-DSDSM_PROFILE): device buffer of 8 int64 cycle counters per candidate, see DESIGN.md.
extern "C" int sdsm_set_debug_buffer(void *d_buf) { g_prof = (long long *)d_buf; return SDSM_OK; }

#ifndef SDSM_HESS_THR
#define SDSM_HESS_THR 0.1f    // same constant as the oracle's ORC_HESS_THR
#endif
static std::atomic<int> g_solver_diag{0};      // sdsm_set_solver_diagnostics (process-wide)
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

// Kernel arguments of a plan laid out in the caller's workspace (the pointers of the blocks by integer arithmetic: a null workspace gives the offsets).
BatchParams make_params(const sdsm_plan *p, void *d_ws)
{
    const uintptr_t b = (uintptr_t)d_ws;
    BatchParams P{};
    P.n = p->n; P.n_total = p->n; P.latency = p->mode == 1; P.n_images = (int)p->images.size();
    for (size_t i = 0; i < p->images.size(); i++) { P.img[i].H = p->images[i].H; P.img[i].W = p->images[i].W; }   // device pointers: filled by the launch
    P.k = p->k; P.R = p->R; P.subsample = p->cfg.smooth_subsample; P.zcap = p->zcap; P.zcap_run = p->zcap_run; P.zshift = p->zshift; P.no_deform = p->no_deform; P.no_trivial_rule = p->cfg.flags & 1;
    P.init_elliptical = p->cfg.init_elliptical; P.max_iters = p->cfg.max_iters; P.k1_pixmax = p->wide_pixels; P.boost_pixels = p->boost_pixels; P.rows_mcap = p->rows_mcap; P.solver_diag = g_solver_diag.load(std::memory_order_relaxed);
    P.light_emax = light_limit(p); P.wide_rest = p->wide_rest;
    P.scale = p->cfg.scale; P.epsilon = p->cfg.epsilon; P.alpha = p->cfg.alpha; P.reg_unit = p->cfg.alpha * std::sqrt(p->cfg.epsilon);
    P.hess_thr = SDSM_HESS_THR;
#define X(name, T, count) P.name = (T *)(b + p->ws_off[WS_##name]);
    SDSM_WS_BLOCKS(X)
#undef X
    P.wide_ticket = (int32_t *)(b + p->ws_off[WS_words] + offsetof(LaunchWords, ticket)); P.wide_timeout = g_wide_timeout;
    P.cls_count = (int32_t *)(b + p->ws_off[WS_words] + offsetof(LaunchWords, list_head));
    P.prof = g_prof; P.prof2 = g_prof ? g_prof + (size_t)16 * p->n : nullptr;
    P.x0 = p->x0;
    return P;
}

// Diagnostic: the kernel arguments over a null workspace (every workspace pointer = its block's offset) and the candidate descriptors, as raw bytes.
extern "C" int sdsm_plan_image(const sdsm_plan *p, void *params, size_t params_bytes, void *cand, size_t cand_bytes)
{
    if (!p || !params || (!cand && p->n > 0)) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_image: null argument");
    if (params_bytes != sizeof(BatchParams) || cand_bytes != sizeof(CandDesc) * (size_t)p->n) return fail(SDSM_ERR_ARGUMENT, "sdsm_plan_image: a buffer is not of the size of what it receives");
    const BatchParams P = make_params(p, nullptr);
    memcpy(params, &P, sizeof(P));
    copy_out(cand, p->cand);
    return SDSM_OK;
}
