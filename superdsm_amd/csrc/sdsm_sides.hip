// The process-wide pool of side streams and its queue probing: which pool streams a caller's stream forks the solve classes onto
// (acquire_sides, choose_sides; used by sdsm_batch_launch_multi in sdsm_api.hip), and the two report entry points.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sdsm_sides.h"

// ONE set per device, shared by all plans and created at the first launch that needs it: the runtime maps streams onto GPU_MAX_HW_QUEUES
// hardware queues in the order of their creation, and side streams created per live plan (the tenth stream of the process and later) came to share
// queues with the caller's stream or among themselves -- the classes of one launch then ran one after the other (NIH3T3-like launch inside the full
// bench run 8.3 instead of 6.4 ms).  One fixed set is no better off once the caller has streams of its own (the step of 8 different images from a
// stream of PyTorch's pool: classes 1b and 2 on one queue, 10.1 instead of 6.4 ms): hence the pool and the choice per caller stream below.
// Launches enqueue under the set's mutex (fork and join events belong to the set); launches from different caller streams share the pool.
static std::mutex g_pool_mutex;
static std::vector<SideSet *> g_side_sets;

hipError_t acquire_sides(const sdsm_plan *p, hipStream_t caller)
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
hipError_t choose_sides(SideSet *q, hipStream_t caller, int want, SideChoice *out)
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
