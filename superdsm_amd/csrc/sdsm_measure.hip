// Per-object measurement tables on the GPU: one sdsm_measure_record per object (bit-packed fragments) or per label (label maps),
// for one image or a set of images.  No reference counterpart beyond a test helper (tests/regression/validate.py:31-36: area and
// centre of mass per label) and one regionprops(...).eccentricity call (superdsm/postprocess.py:340-344); the definition every kernel
// is tested against is the host code of superdsm_amd/measure.py.
//
//   k_absmax            max finite |g| per image (integer atomic on the bits of a non-negative double), from which the measuring
//                       kernels take the exponent e of the image's intensity quantum 2^(e - 62) without a host round trip
//   k_measure_objects   one workgroup per object: the set bits of the fragment (each_set_bit of sdsm_tables.h), 64-bit sums in registers, one reduction of the
//                       workgroup through LDS, no global atomics
//   k_measure_labels    one workgroup per band of LBAND consecutive pixels (raster order) of one image: a thread owns segments of LSEG
//                       pixels and keeps the sums of its current label in registers while the label does not change; on a change
//                       it flushes into an LDS table keyed by label (lds_label_slot of sdsm_tables.h, 64-bit LDS adds);
//                       the occupied slots go to the global records by 64-bit integer atomics at the end of the band.  A label
//                       without a free slot goes straight to the global atomics.
//   k_labels_init / k_labels_finish   the identities of the atomics before, the record's final form after
//   k_overlap_pairs     the contingency table of two label maps (superdsm_amd/compare.py): the bands and segments of k_measure_labels over
//                       both maps; a thread keeps its current pair (a, b) and the length of its run in registers and flushes on a change
//                       into an LDS table keyed by the 64-bit pair (64-bit LDS compare-and-swap, 32-bit counts); the occupied slots go
//                       to the image's global hash table (pair_table_slot of sdsm_tables.h, 64-bit counts) at the end of the band.  A
//                       pair without an LDS slot goes straight there; one without a global slot is counted and dropped, never waited for.
//
//   k_label_pixel_counts / k_label_starts / k_label_pixel_lists   boundary distances (superdsm_amd/boundary.py): per label its pixels and
//                       boundary pixels (bands and segments as above, an LDS table keyed by label), the exclusive sum of the counts, and
//                       every label's pixels scattered into one coordinate list, boundary pixels first (one atomic per run and part)
//   k_pair_init / k_pair_distances   one workgroup per (pair of labels, phase, chunk of query pixels): the target's boundary list goes
//                       through LDS in tiles, a lane keeps the 32-bit integer minima of its query pixels, q = floor(sqrt(d2 * 2^32))
//                       once per query pixel, wavefront reductions, integer atomicMax / 64-bit atomicAdd into the pair's record
//
// Every sum over pixels is an integer sum and every atomic an integer add / min / max / or, so the bytes do not depend on the order,
// the launch or the set size.  Intensities enter as q = rint(ldexp(g, 62 - e)) in two limbs (bits 0-31, and q >> 32).
#include "sdsm_tables.h"
#include <climits>
#include <cmath>

namespace {

constexpr int MTPB = 256;
constexpr int ABS_PIX = 2048;                    // k_absmax: pixels per workgroup
constexpr int LSEG = 16;                         // k_measure_labels: consecutive pixels of a thread's segment (64 B of labels)
constexpr int LBAND = 16384;                     //   pixels of a band: 4 segments per thread
constexpr int LBITS = 8;
constexpr int LSLOTS = 1 << LBITS;               //   slots of the LDS table (28 KB: 5 workgroups per compute unit)
constexpr int LPROBES = 16;                      //   slots tried before a label goes to the global atomics
constexpr int FIN_RECS = MTPB;                   // k_labels_init / k_labels_finish: records per workgroup
// k_overlap_pairs: the LDS table of a band.  A slot is 12 bytes (64-bit key, 32-bit count), so 1024 slots are 12 KB: a compute unit holds
// 32 waves = 8 workgroups of 256 threads, 96 KB of its 160 KB of LDS, and the wave slots bound the occupancy, not the table (2048 slots
// would: 8 x 24 KB = 192 KB).  A band meets few pairs: 16 384 pixels are 23 rows of a 520 x 696 image or 4 rows of a 4096-wide one, and
// objects of radius 15 leave about 100 (object, object) and (object, background) pairs there, a load of 0.1.  At a load a of the table
// an insertion of a new key tries (1 + 1 / (1 - a)^2) / 2 slots on average (linear probing): 1.1 at a = 0.1, 2.5 at a = 0.5, and 8
// tries fail only behind a cluster of 8 occupied slots, which needs a load near 0.7 (700 pairs in a band) to become common.  Such a
// pair goes straight to the global table: the result does not depend on either constant, only the time does.
constexpr int OBITS = 10;
constexpr int OSLOTS = 1 << OBITS;               //   slots of the LDS table
constexpr int OPROBES = 8;                       //   slots tried before a pair goes to the global table

// the sums of a set of pixels, and how two of them combine
struct Acc {
    i64 area, sum_r, sum_c, n_finite, ghi;
    u64 sum_rr, sum_rc, sum_cc, glo, kmin, kmax;     // kmin / kmax: monotone keys of gmin / gmax
    int32_t r0, c0, r1, c1, flags;
};

__device__ __forceinline__ void acc_clear(Acc &a)
{
    a.area = a.sum_r = a.sum_c = a.n_finite = a.ghi = 0;
    a.sum_rr = a.sum_rc = a.sum_cc = a.glo = 0;
    a.kmin = ~0ull; a.kmax = 0;
    a.r0 = a.c0 = INT_MAX; a.r1 = a.c1 = 0; a.flags = 0;
}

__device__ __forceinline__ void acc_pixel(Acc &a, int r, int c)
{
    a.area++;
    a.sum_r += r; a.sum_c += c;
    a.sum_rr += (u64)((uint32_t)r * (uint32_t)r);           // r, c <= 65534: the products fit 32 bits
    a.sum_rc += (u64)((uint32_t)r * (uint32_t)c);
    a.sum_cc += (u64)((uint32_t)c * (uint32_t)c);
    a.r0 = r < a.r0 ? r : a.r0; a.r1 = r + 1 > a.r1 ? r + 1 : a.r1;
    a.c0 = c < a.c0 ? c : a.c0; a.c1 = c + 1 > a.c1 ? c + 1 : a.c1;
}

__device__ __forceinline__ void acc_intensity(Acc &a, double g, int shift)
{
    const u64 b = (u64)__double_as_longlong(g);
    if (((b >> 52) & 0x7ff) == 0x7ff) { a.flags |= 2; return; }     // inf / NaN: counted by the flag, adds nothing
    const i64 q = (i64)rint(ldexp(g, shift));                        // |q| <= 2^62
    a.n_finite++;
    a.glo += (u64)(uint32_t)q;
    a.ghi += q >> 32;
    const u64 k = dkey(g);
    a.kmin = k < a.kmin ? k : a.kmin; a.kmax = k > a.kmax ? k : a.kmax;
}

__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b)
{
    a.area += b.area; a.sum_r += b.sum_r; a.sum_c += b.sum_c; a.n_finite += b.n_finite; a.ghi += b.ghi;
    a.sum_rr += b.sum_rr; a.sum_rc += b.sum_rc; a.sum_cc += b.sum_cc; a.glo += b.glo;
    a.kmin = b.kmin < a.kmin ? b.kmin : a.kmin; a.kmax = b.kmax > a.kmax ? b.kmax : a.kmax;
    a.r0 = b.r0 < a.r0 ? b.r0 : a.r0; a.c0 = b.c0 < a.c0 ? b.c0 : a.c0;
    a.r1 = b.r1 > a.r1 ? b.r1 : a.r1; a.c1 = b.c1 > a.c1 ? b.c1 : a.c1;
    a.flags |= b.flags;
}

__device__ __forceinline__ Acc acc_shfl_down(const Acc &a, int o)
{
    Acc b;
    b.area = __shfl_down(a.area, o); b.sum_r = __shfl_down(a.sum_r, o); b.sum_c = __shfl_down(a.sum_c, o);
    b.n_finite = __shfl_down(a.n_finite, o); b.ghi = __shfl_down(a.ghi, o);
    b.sum_rr = __shfl_down(a.sum_rr, o); b.sum_rc = __shfl_down(a.sum_rc, o); b.sum_cc = __shfl_down(a.sum_cc, o);
    b.glo = __shfl_down(a.glo, o); b.kmin = __shfl_down(a.kmin, o); b.kmax = __shfl_down(a.kmax, o);
    b.r0 = __shfl_down(a.r0, o); b.c0 = __shfl_down(a.c0, o); b.r1 = __shfl_down(a.r1, o); b.c1 = __shfl_down(a.c1, o);
    b.flags = __shfl_down(a.flags, o);
    return b;
}

// the record of a set of pixels of an H x W image (area == 0: the zero record)
__device__ __forceinline__ void write_record(sdsm_measure_record *out, const Acc &a, int H, int W, int e)
{
    sdsm_measure_record R;
    const bool any = a.area > 0;
    R.area = a.area; R.sum_r = a.sum_r; R.sum_c = a.sum_c;
    R.sum_rr = a.sum_rr; R.sum_rc = a.sum_rc; R.sum_cc = a.sum_cc;
    R.r0 = any ? a.r0 : 0; R.c0 = any ? a.c0 : 0; R.r1 = any ? a.r1 : 0; R.c1 = any ? a.c1 : 0;
    R.flags = any ? ((a.flags & 2) | ((a.r0 == 0 || a.c0 == 0 || a.r1 == H || a.c1 == W) ? 1 : 0)) : 0;
    R.scale_exp = e;
    R.n_finite = a.n_finite; R.gsum_lo = a.glo; R.gsum_hi = a.ghi;
    R.gmin = a.n_finite > 0 ? dkey_inv(a.kmin) : __longlong_as_double(0x7ff0000000000000ll);
    R.gmax = a.n_finite > 0 ? dkey_inv(a.kmax) : __longlong_as_double((i64)0xfff0000000000000ull);
    *out = R;
}

// ---- max finite |g| per image ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MTPB) void k_absmax(SetLabels S, const double *g_, u64 *maxbits)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int64_t px = (int64_t)S.H[im] * S.W[im];
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * ABS_PIX;
    const double *g = g_ + S.off[im];
    u64 m = 0;
    for (int e = threadIdx.x; e < ABS_PIX; e += MTPB) {
        const int64_t p = p0 + e;
        if (p >= px) break;
        const u64 b = (u64)__double_as_longlong(g[p]) & ~(1ull << 63);
        if ((b >> 52) != 0x7ff && b > m) m = b;
    }
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_down(m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(maxbits + im, m);
}

__global__ __launch_bounds__(MTPB) void k_scale_exp(int n, const u64 *maxbits, int32_t *out)
{
    const int i = blockIdx.x * MTPB + threadIdx.x;
    if (i < n) out[i] = maxbits ? scale_exp(maxbits[i]) : 0;
}

// ---- objects: one workgroup per fragment ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MTPB) void k_measure_objects(SetLabels S, const int32_t *obj_image, const int32_t *boxes, const int64_t *bits_off,
                                                          const uint32_t *bits_, const double *g_, const u64 *maxbits, sdsm_measure_record *out)
{
    __shared__ Acc part[MTPB / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int im = obj_image ? obj_image[i] : 0;
    Acc a;
    acc_clear(a);
    Fragment f;
    const bool inside = fragment_box(S, im, boxes, i, f);
    const int e = g_ && f.H > 0 ? scale_exp(maxbits[im]) : 0;                    // (f.H == 0: `im` is no image of the set)
    if (inside) {                                // a box that leaves its image gives the zero record: no pixel outside is read
        const double *g = g_ ? g_ + S.off[im] : nullptr;
        each_set_bit<MTPB>(bits_ + bits_off[i], f, tid, [&](uint32_t, int r, int c) {
            acc_pixel(a, r, c);
            if (g) acc_intensity(a, g[(int64_t)r * f.W + c], 62 - e);
        });
    }
    for (int o = 32; o > 0; o >>= 1) acc_merge(a, acc_shfl_down(a, o));
    if ((tid & 63) == 0) part[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < MTPB / 64; k++) acc_merge(a, part[k]);
        write_record(out + i, a, f.H, f.W, e);
    }
}

// ---- labels ------------------------------------------------------------------------------------------------------------------------
// While the atomics run, a record holds their identities and partial results: r0 / c0 INT_MAX, gmin / gmax as keys; k_labels_finish
// gives it its final form.
__global__ __launch_bounds__(MTPB) void k_labels_init(SetLabels S, sdsm_measure_record *recs, int32_t *bad)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int l = (blockIdx.x - S.start[im]) * FIN_RECS + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < S.n) bad[threadIdx.x] = 0;
    if (l >= S.n_labels[im]) return;
    sdsm_measure_record R;
    R.area = R.sum_r = R.sum_c = 0; R.sum_rr = R.sum_rc = R.sum_cc = 0;
    R.r0 = R.c0 = INT_MAX; R.r1 = R.c1 = 0; R.flags = 0; R.scale_exp = 0;
    R.n_finite = 0; R.gsum_lo = 0; R.gsum_hi = 0;
    R.gmin = __longlong_as_double(-1ll); R.gmax = __longlong_as_double(0ll);      // keys: ~0 and 0
    recs[S.rec_off[im] + l] = R;
}

__global__ __launch_bounds__(MTPB) void k_labels_finish(SetLabels S, sdsm_measure_record *recs, const u64 *maxbits)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int l = (blockIdx.x - S.start[im]) * FIN_RECS + threadIdx.x;
    if (l >= S.n_labels[im]) return;
    sdsm_measure_record *R = recs + S.rec_off[im] + l;
    Acc a;
    a.area = R->area; a.sum_r = R->sum_r; a.sum_c = R->sum_c; a.n_finite = R->n_finite; a.ghi = R->gsum_hi;
    a.sum_rr = R->sum_rr; a.sum_rc = R->sum_rc; a.sum_cc = R->sum_cc; a.glo = R->gsum_lo;
    a.kmin = (u64)__double_as_longlong(R->gmin); a.kmax = (u64)__double_as_longlong(R->gmax);
    a.r0 = R->r0; a.c0 = R->c0; a.r1 = R->r1; a.c1 = R->c1; a.flags = R->flags;
    write_record(R, a, S.H[im], S.W[im], maxbits ? scale_exp(maxbits[im]) : 0);
}

// the sums of one label into its global record, by integer atomics (zero terms are left out)
__device__ __forceinline__ void emit_global(sdsm_measure_record *R, const Acc &a)
{
    atomicAdd((u64 *)&R->area, (u64)a.area);
    atomicAdd((u64 *)&R->sum_r, (u64)a.sum_r);
    atomicAdd((u64 *)&R->sum_c, (u64)a.sum_c);
    atomicAdd((u64 *)&R->sum_rr, a.sum_rr);
    atomicAdd((u64 *)&R->sum_rc, a.sum_rc);
    atomicAdd((u64 *)&R->sum_cc, a.sum_cc);
    atomicMin(&R->r0, a.r0); atomicMin(&R->c0, a.c0);
    atomicMax(&R->r1, a.r1); atomicMax(&R->c1, a.c1);
    if (a.flags) atomicOr(&R->flags, a.flags);
    if (a.n_finite) {
        atomicAdd((u64 *)&R->n_finite, (u64)a.n_finite);
        atomicAdd((u64 *)&R->gsum_lo, a.glo);
        atomicAdd((u64 *)&R->gsum_hi, (u64)a.ghi);
        atomicMin((u64 *)&R->gmin, a.kmin);
        atomicMax((u64 *)&R->gmax, a.kmax);
    }
}

struct LTable {                                  // the per-workgroup table, one array per field: a slot is one index
    int32_t key[LSLOTS];                         // -1: free
    u64 area[LSLOTS], sum_r[LSLOTS], sum_c[LSLOTS], sum_rr[LSLOTS], sum_rc[LSLOTS], sum_cc[LSLOTS];
    u64 n_finite[LSLOTS], glo[LSLOTS], ghi[LSLOTS], kmin[LSLOTS], kmax[LSLOTS];
    int32_t r0[LSLOTS], c0[LSLOTS], r1[LSLOTS], c1[LSLOTS], flags[LSLOTS];
};

__device__ __forceinline__ void flush_label(LTable &T, int32_t label, const Acc &a, sdsm_measure_record *recs)
{
    const bool found = lds_label_slot<LBITS, LPROBES>(T.key, label, [&](uint32_t s) {
        atomicAdd(&T.area[s], (u64)a.area);
        atomicAdd(&T.sum_r[s], (u64)a.sum_r);
        atomicAdd(&T.sum_c[s], (u64)a.sum_c);
        atomicAdd(&T.sum_rr[s], a.sum_rr);
        atomicAdd(&T.sum_rc[s], a.sum_rc);
        atomicAdd(&T.sum_cc[s], a.sum_cc);
        atomicMin(&T.r0[s], a.r0); atomicMin(&T.c0[s], a.c0);
        atomicMax(&T.r1[s], a.r1); atomicMax(&T.c1[s], a.c1);
        if (a.flags) atomicOr(&T.flags[s], a.flags);
        if (a.n_finite) {
            atomicAdd(&T.n_finite[s], (u64)a.n_finite);
            atomicAdd(&T.glo[s], a.glo);
            atomicAdd(&T.ghi[s], (u64)a.ghi);
            atomicMin(&T.kmin[s], a.kmin);
            atomicMax(&T.kmax[s], a.kmax);
        }
    });
    if (!found) emit_global(recs + label, a);            // no slot: correct and slow
}

__global__ __launch_bounds__(MTPB) void k_measure_labels(SetLabels S, const int32_t *labels_, const double *g_, const u64 *maxbits,
                                                         sdsm_measure_record *recs_, int32_t *bad)
{
    __shared__ LTable T;
    static_assert(LBAND % (LSEG * MTPB) == 0, "band size");
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int W = S.W[im], n_labels = S.n_labels[im];
    const int64_t px = (int64_t)S.H[im] * W;
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * LBAND;
    const int32_t *lab = labels_ + S.off[im];
    const double *g = g_ ? g_ + S.off[im] : nullptr;
    sdsm_measure_record *recs = recs_ + S.rec_off[im];
    const int shift = 62 - (g ? scale_exp(maxbits[im]) : 0);
    for (int s = tid; s < LSLOTS; s += MTPB) {
        T.key[s] = -1;
        T.area[s] = T.sum_r[s] = T.sum_c[s] = T.sum_rr[s] = T.sum_rc[s] = T.sum_cc[s] = 0;
        T.n_finite[s] = T.glo[s] = T.ghi[s] = 0; T.kmin[s] = ~0ull; T.kmax[s] = 0;
        T.r0[s] = T.c0[s] = INT_MAX; T.r1[s] = T.c1[s] = 0; T.flags[s] = 0;
    }
    __syncthreads();
    Acc a;
    acc_clear(a);
    int32_t cur = -1;                            // the label whose sums the registers hold; -1: none
    int n_bad = 0;
    for (int it = 0; it < LBAND / (LSEG * MTPB); it++) {
        const int64_t q0 = p0 + ((int64_t)it * MTPB + tid) * LSEG;
        if (q0 >= px) break;
        const int n = px - q0 < LSEG ? (int)(px - q0) : LSEG;
        const bool vec = n == LSEG && (((uintptr_t)(lab + q0)) & 15) == 0;       // 16-byte loads where the segment is whole and aligned
        int r = (int)(q0 / W), c = (int)(q0 % W);
        int4 t = make_int4(0, 0, 0, 0);
#pragma unroll 1
        for (int k = 0; k < n; k++) {            // (one flush site: the loop stays rolled)
            if ((k & 3) == 0) {
                if (vec) t = *(const int4 *)(lab + q0 + k);
                else { t.x = lab[q0 + k]; t.y = k + 1 < n ? lab[q0 + k + 1] : 0; t.z = k + 2 < n ? lab[q0 + k + 2] : 0; t.w = k + 3 < n ? lab[q0 + k + 3] : 0; }
            }
            const int32_t l = (k & 3) == 0 ? t.x : (k & 3) == 1 ? t.y : (k & 3) == 2 ? t.z : t.w;
            if (l != cur) {
                if (cur >= 0) flush_label(T, cur, a, recs);
                acc_clear(a);
                cur = (l >= 0 && l < n_labels) ? l : -1;
            }
            if (cur >= 0) {
                acc_pixel(a, r, c);
                if (g) acc_intensity(a, g[q0 + k], shift);
            } else {
                n_bad++;
            }
            if (++c == W) { c = 0; r++; }
        }
    }
    if (cur >= 0) flush_label(T, cur, a, recs);
    if (n_bad) atomicAdd(bad + im, n_bad);
    __syncthreads();
    for (int s = tid; s < LSLOTS; s += MTPB) {
        const int32_t label = T.key[s];
        if (label < 0) continue;
        Acc t;
        t.area = (i64)T.area[s]; t.sum_r = (i64)T.sum_r[s]; t.sum_c = (i64)T.sum_c[s]; t.n_finite = (i64)T.n_finite[s]; t.ghi = (i64)T.ghi[s];
        t.sum_rr = T.sum_rr[s]; t.sum_rc = T.sum_rc[s]; t.sum_cc = T.sum_cc[s]; t.glo = T.glo[s]; t.kmin = T.kmin[s]; t.kmax = T.kmax[s];
        t.r0 = T.r0[s]; t.c0 = T.c0[s]; t.r1 = T.r1[s]; t.c1 = T.c1[s]; t.flags = T.flags[s];
        emit_global(recs + label, t);
    }
}

// ---- contingency table of two label maps ---------------------------------------------------------------------------------------------
struct OCap { int64_t cap[SDSM_MAX_SET_IMAGES]; };          // slots of each image's global table, a power of two

__device__ __forceinline__ u64 pair_hash(u64 key)           // multiplicative: the high bits depend on every bit of the key
{
    return key * 0x9E3779B97F4A7C15ull;
}

// n pixels of the pair `key` into the global table of its image (pair_table_slot); a pair that finds the table full is counted in
// status[1] and its pixels are dropped
__device__ __forceinline__ void insert_global(u64 *keys, u64 *counts, int64_t cap, u64 key, u64 n, int32_t *status)
{
    const u64 h = pair_hash(key);
    if (!pair_table_slot(keys, cap, (h ^ (h >> 31)) & ((u64)cap - 1), key, [&](u64 s) { atomicAdd(counts + s, n); })) atomicAdd(status + 1, 1);
}

struct OTable {                                  // the per-workgroup table
    u64 key[OSLOTS];                             // PAIR_FREE: free
    uint32_t count[OSLOTS];                      // a band holds LBAND = 16 384 pixels
};

__device__ __forceinline__ void flush_pair(OTable &T, u64 key, uint32_t n, u64 *keys, u64 *counts, int64_t cap, int32_t *status)
{
    uint32_t s = (uint32_t)(pair_hash(key) >> (64 - OBITS));
    for (int k = 0; k < OPROBES; k++, s = (s + 1) & (OSLOTS - 1)) {
        const u64 old = atomicCAS(&T.key[s], PAIR_FREE, key);
        if (old != PAIR_FREE && old != key) continue;
        atomicAdd(&T.count[s], n);
        return;
    }
    insert_global(keys, counts, cap, key, n, status);        // no slot: correct and slow
}

// S.rec_off: first slot of the image's global table; status: per image [0] pixels with a negative label (skipped), [1] pairs without a slot
__global__ __launch_bounds__(MTPB) void k_overlap_pairs(SetLabels S, OCap C, const int32_t *a_, const int32_t *b_, u64 *keys_, u64 *counts_, int32_t *status_)
{
    __shared__ OTable T;
    static_assert(LBAND % (LSEG * MTPB) == 0 && LBAND <= 0xffffffffll, "band size and the 32-bit counts of the LDS table");
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int64_t px = (int64_t)S.H[im] * S.W[im];
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * LBAND;
    const int32_t *la = a_ + S.off[im], *lb = b_ + S.off[im];
    u64 *keys = keys_ + S.rec_off[im], *counts = counts_ + S.rec_off[im];
    const int64_t cap = C.cap[im];
    int32_t *status = status_ + 2 * im;
    for (int s = tid; s < OSLOTS; s += MTPB) { T.key[s] = PAIR_FREE; T.count[s] = 0; }
    __syncthreads();
    u64 cur = PAIR_FREE;                             // the pair whose run the registers hold; PAIR_FREE: none
    uint32_t run = 0;
    int n_bad = 0;
    for (int it = 0; it < LBAND / (LSEG * MTPB); it++) {
        const int64_t q0 = p0 + ((int64_t)it * MTPB + tid) * LSEG;
        if (q0 >= px) break;
        const int n = px - q0 < LSEG ? (int)(px - q0) : LSEG;
        const bool vec = n == LSEG && ((((uintptr_t)(la + q0)) | ((uintptr_t)(lb + q0))) & 15) == 0;      // 16-byte loads where both segments are whole and aligned
        int4 t = make_int4(0, 0, 0, 0), u = make_int4(0, 0, 0, 0);
#pragma unroll 1
        for (int k = 0; k < n; k++) {            // (one flush site: the loop stays rolled)
            if ((k & 3) == 0) {
                if (vec) { t = *(const int4 *)(la + q0 + k); u = *(const int4 *)(lb + q0 + k); }
                else {
                    t.x = la[q0 + k]; t.y = k + 1 < n ? la[q0 + k + 1] : 0; t.z = k + 2 < n ? la[q0 + k + 2] : 0; t.w = k + 3 < n ? la[q0 + k + 3] : 0;
                    u.x = lb[q0 + k]; u.y = k + 1 < n ? lb[q0 + k + 1] : 0; u.z = k + 2 < n ? lb[q0 + k + 2] : 0; u.w = k + 3 < n ? lb[q0 + k + 3] : 0;
                }
            }
            const int32_t x = (k & 3) == 0 ? t.x : (k & 3) == 1 ? t.y : (k & 3) == 2 ? t.z : t.w;
            const int32_t y = (k & 3) == 0 ? u.x : (k & 3) == 1 ? u.y : (k & 3) == 2 ? u.z : u.w;
            if ((x | y) < 0) { n_bad++; continue; }          // skipped; the run of the current pair goes on behind it
            const u64 key = ((u64)(uint32_t)x << 32) | (uint32_t)y;
            if (key != cur) {
                if (run) flush_pair(T, cur, run, keys, counts, cap, status);
                cur = key;
                run = 0;
            }
            run++;
        }
    }
    if (run) flush_pair(T, cur, run, keys, counts, cap, status);
    if (n_bad) atomicAdd(status, n_bad);
    __syncthreads();
    for (int s = tid; s < OSLOTS; s += MTPB)     // one lane per slot
        if (T.key[s] != PAIR_FREE) insert_global(keys, counts, cap, T.key[s], T.count[s], status);
}

void grid_pixels(SetLabels &S, int per_block)
{
    for (int i = 0; i < S.n; i++) S.start[i + 1] = S.start[i] + (int32_t)(((int64_t)S.H[i] * S.W[i] + per_block - 1) / per_block);
}

void grid_records(SetLabels &S)
{
    for (int i = 0; i < S.n; i++) S.start[i + 1] = S.start[i] + (S.n_labels[i] + FIN_RECS - 1) / FIN_RECS;
}

// max finite |g| per image into d_gmax_abs (the bits of a non-negative double are ordered as integers) and e into d_scale_exp
hipError_t launch_scale(SetLabels S, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp, hipStream_t stream)
{
    if (d_g) {
        hipError_t e = hipMemsetAsync(d_gmax_abs, 0, (size_t)S.n * sizeof(double), stream);
        if (e != hipSuccess) return e;
        grid_pixels(S, ABS_PIX);
        hipLaunchKernelGGL(k_absmax, dim3(S.start[S.n]), dim3(MTPB), 0, stream, S, d_g, (u64 *)d_gmax_abs);
    }
    if (d_scale_exp) hipLaunchKernelGGL(k_scale_exp, dim3(1), dim3(MTPB), 0, stream, S.n, d_g ? (const u64 *)d_gmax_abs : nullptr, d_scale_exp);
    return hipGetLastError();
}

// ---- boundary distances between two label maps -----------------------------------------------------------------------------------------
constexpr int BMAXL = SDSM_BOUNDARY_MAX_LABELS;
constexpr int BBITS = 10;
constexpr int BSLOTS = 1 << BBITS;               // k_label_pixel_counts: slots of the LDS table (12 KB, as k_overlap_pairs)
constexpr int BPROBES = 8;                       //   slots tried before a label goes to the global atomics
constexpr int DTILE = SDSM_BOUNDARY_TILE;        // k_pair_distances: target pixels per LDS tile (8 KB as (row, column) pairs)
constexpr int DCHUNK = SDSM_BOUNDARY_CHUNK;      //   query pixels of a workgroup
constexpr int DQ = DCHUNK / MTPB;                //   query pixels of a lane
static_assert(DCHUNK % MTPB == 0 && BMAXL % MTPB == 0 && BMAXL <= 65536, "chunk and label range");

// one of the 4-neighbours of pixel p = (r, c) inside the image carries another label than l
__device__ __forceinline__ bool on_boundary(const int32_t *lab, int64_t p, int r, int c, int H, int W, int32_t l)
{
    return (r > 0 && lab[p - W] != l) || (r + 1 < H && lab[p + W] != l) || (c > 0 && lab[p - 1] != l) || (c + 1 < W && lab[p + 1] != l);
}

struct BTable {                                  // the per-workgroup table of k_label_pixel_counts
    int32_t key[BSLOTS];                         // -1: free
    uint32_t area[BSLOTS], edge[BSLOTS];
};

__device__ __forceinline__ void flush_counts(BTable &T, int32_t label, uint32_t area, uint32_t edge, int32_t *counts)
{
    const bool found = lds_label_slot<BBITS, BPROBES>(T.key, label, [&](uint32_t s) {
        atomicAdd(&T.area[s], area);
        if (edge) atomicAdd(&T.edge[s], edge);
    });
    if (!found) {                                // no slot: correct and slow
        atomicAdd(counts + 2 * label, (int32_t)area);
        if (edge) atomicAdd(counts + 2 * label + 1, (int32_t)edge);
    }
}

// the bands and segments of k_measure_labels; a thread keeps the counts of its current label in registers while the label does not change
__global__ __launch_bounds__(MTPB) void k_label_pixel_counts(SetLabels S, const int32_t *labels_, int32_t *counts_, int32_t *bad)
{
    __shared__ BTable T;
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int H = S.H[im], W = S.W[im];
    const int64_t px = (int64_t)H * W;
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * LBAND;
    const int32_t *lab = labels_ + S.off[im];
    int32_t *counts = counts_ + (int64_t)im * 2 * BMAXL;
    for (int s = tid; s < BSLOTS; s += MTPB) { T.key[s] = -1; T.area[s] = T.edge[s] = 0; }
    __syncthreads();
    int32_t cur = -1;                            // the label whose counts the registers hold; -1: none
    uint32_t area = 0, edge = 0;
    int n_bad = 0;
    for (int it = 0; it < LBAND / (LSEG * MTPB); it++) {
        const int64_t q0 = p0 + ((int64_t)it * MTPB + tid) * LSEG;
        if (q0 >= px) break;
        const int n = px - q0 < LSEG ? (int)(px - q0) : LSEG;
        int r = (int)(q0 / W), c = (int)(q0 % W);
#pragma unroll 1
        for (int k = 0; k < n; k++) {
            const int32_t l = lab[q0 + k];
            if (l != cur) {
                if (cur >= 0) flush_counts(T, cur, area, edge, counts);
                area = edge = 0;
                cur = (l >= 0 && l < BMAXL) ? l : -1;
            }
            if (cur >= 0) {
                area++;
                if (cur != 0 && on_boundary(lab, q0 + k, r, c, H, W, cur)) edge++;
            } else {
                n_bad++;
            }
            if (++c == W) { c = 0; r++; }
        }
    }
    if (cur >= 0) flush_counts(T, cur, area, edge, counts);
    if (n_bad) atomicAdd(bad + im, n_bad);
    __syncthreads();
    for (int s = tid; s < BSLOTS; s += MTPB) {
        const int32_t label = T.key[s];
        if (label < 0) continue;
        atomicAdd(counts + 2 * label, (int32_t)T.area[s]);
        if (T.edge[s]) atomicAdd(counts + 2 * label + 1, (int32_t)T.edge[s]);
    }
}

// one workgroup per image: every label >= 1 gets its own range of the image's list (fewer than 2^30 entries in all), and the cursors of the
// scatter are cleared.  Thread t lays the labels t, t + 256, ... one behind the other (coalesced reads and writes), behind the ranges of
// the threads before it: the ranges are disjoint and dense, their order is not that of the labels.
__global__ __launch_bounds__(MTPB) void k_label_starts(const int32_t *counts_, int32_t *start_, int32_t *cursor_)
{
    __shared__ int32_t part[MTPB];
    const int tid = threadIdx.x;
    const int2 *counts = (const int2 *)(counts_ + (int64_t)blockIdx.x * 2 * BMAXL);
    int32_t *start = start_ + (int64_t)blockIdx.x * BMAXL;
    int2 *cursor = (int2 *)(cursor_ + (int64_t)blockIdx.x * 2 * BMAXL);
    int32_t s = 0;
    for (int l = tid; l < BMAXL; l += MTPB) s += l ? counts[l].x : 0;
    part[tid] = s;
    __syncthreads();
    int32_t base = 0;
    for (int k = 0; k < tid; k++) base += part[k];
    for (int l = tid; l < BMAXL; l += MTPB) {
        start[l] = base;
        base += l ? counts[l].x : 0;
        cursor[l] = make_int2(0, 0);
    }
}

// A thread walks its segments run by run: the boundary pixels of a run of one label as a bit mask, one atomic per run and part of the
// label's list, then the coordinates.  An entry past the image's part of the list (counts of another map) is dropped, never written.
__global__ __launch_bounds__(MTPB) void k_label_pixel_lists(SetLabels S, const int32_t *labels_, const int32_t *counts_, const int32_t *start_,
                                                            int32_t *cursor_, uint32_t *list_)
{
    static_assert(LSEG <= 32, "the boundary mask of a run");
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int H = S.H[im], W = S.W[im];
    const int64_t px = (int64_t)H * W;
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * LBAND;
    const int32_t *lab = labels_ + S.off[im];
    const int32_t *counts = counts_ + (int64_t)im * 2 * BMAXL, *start = start_ + (int64_t)im * BMAXL;
    int32_t *cursor = cursor_ + (int64_t)im * 2 * BMAXL;
    uint32_t *list = list_ + S.off[im];
    for (int it = 0; it < LBAND / (LSEG * MTPB); it++) {
        const int64_t q0 = p0 + ((int64_t)it * MTPB + tid) * LSEG;
        if (q0 >= px) break;
        const int n = px - q0 < LSEG ? (int)(px - q0) : LSEG;
        int r = (int)(q0 / W), c = (int)(q0 % W);
        int k = 0;
        while (k < n) {
            const int32_t l = lab[q0 + k];
            const bool listed = l > 0 && l < BMAXL;
            int k1 = k, rr = r, cc = c;
            uint32_t mask = 0;
            while (k1 < n && lab[q0 + k1] == l) {
                if (listed && on_boundary(lab, q0 + k1, rr, cc, H, W, l)) mask |= 1u << (k1 - k);
                if (++cc == W) { cc = 0; rr++; }
                k1++;
            }
            if (listed) {
                const int nb = __popc(mask), ni = (k1 - k) - nb;
                uint32_t pb = (uint32_t)start[l] + (nb ? (uint32_t)atomicAdd(cursor + 2 * l, nb) : 0u);
                uint32_t pi = (uint32_t)start[l] + (uint32_t)counts[2 * l + 1] + (ni ? (uint32_t)atomicAdd(cursor + 2 * l + 1, ni) : 0u);
                for (int j = k; j < k1; j++) {
                    const uint32_t v = ((uint32_t)r << 16) | (uint32_t)c;
                    const uint32_t pos = ((mask >> (j - k)) & 1u) ? pb++ : pi++;
                    if (pos < (uint64_t)px) list[pos] = v;
                    if (++c == W) { c = 0; r++; }
                }
            } else {
                r = rr; c = cc;
            }
            k = k1;
        }
    }
}

// (q(d2) = floor(sqrt(d2 * 2^32)) is quantised_distance of sdsm_tables.h, which the depth tables take as well)
struct DArgs {
    const int32_t *a, *b, *counts_a, *counts_b, *start_a, *start_b;
    const uint32_t *list_a, *list_b;
};

__device__ __forceinline__ bool pair_ok(const SetImages &S, int im, int la, int lb)
{
    return im >= 0 && im < S.n && la > 0 && la < BMAXL && lb > 0 && lb < BMAXL;
}

__global__ __launch_bounds__(MTPB) void k_pair_init(SetLabels S, DArgs A, int n_pairs, const int32_t *pairs, sdsm_pair_distance *recs)
{
    const int i = blockIdx.x * MTPB + threadIdx.x;
    if (i >= n_pairs) return;
    const int im = pairs[4 * i], la = pairs[4 * i + 1], lb = pairs[4 * i + 2];
    const bool ok = pair_ok(S, im, la, lb);
    sdsm_pair_distance R;
    R.a = la; R.b = lb;
    R.boundary_a = ok ? A.counts_a[(int64_t)im * 2 * BMAXL + 2 * la + 1] : 0;
    R.boundary_b = ok ? A.counts_b[(int64_t)im * 2 * BMAXL + 2 * lb + 1] : 0;
    R.max_d2_ab = R.max_d2_ba = -1;
    R.flags = (R.boundary_a == 0 ? 1 : 0) | (R.boundary_b == 0 ? 2 : 0);
    R.reserved = 0;
    R.sum_q_ab = R.sum_q_ba = R.nsd_num = R.nsd_den = 0;
    recs[i] = R;
}

// One workgroup per item (pair, phase, chunk).  A lane owns DQ query pixels and their running minima; the target's boundary goes through
// LDS in tiles of DTILE pixels, every lane reading the same entry (a broadcast).  Rows and columns differ by less than 2^16, so the
// squares are 24-bit multiplies and their sum fits int32.  q is applied once per query pixel, after the last tile.
__global__ __launch_bounds__(MTPB) void k_pair_distances(SetLabels S, DArgs A, int n_pairs, const int32_t *pairs, const int32_t *items, sdsm_pair_distance *recs)
{
    __shared__ int2 tile[DTILE];
    __shared__ u64 red1[MTPB / 64], red2[MTPB / 64];
    __shared__ int32_t redm[MTPB / 64];
    const int tid = threadIdx.x;
    const int32_t *item = items + 4 * (int64_t)blockIdx.x;
    const int pair = item[0], phase = item[1], chunk = item[2];
    if (pair < 0 || pair >= n_pairs || phase < 0 || phase > 3 || chunk < 0) return;          // (uniform: the whole workgroup leaves)
    const int im = pairs[4 * pair], la = pairs[4 * pair + 1], lb = pairs[4 * pair + 2];
    if (!pair_ok(S, im, la, lb)) return;
    const int H = S.H[im], W = S.W[im];
    const int64_t px = (int64_t)H * W;
    const int32_t *ca = A.counts_a + (int64_t)im * 2 * BMAXL, *cb = A.counts_b + (int64_t)im * 2 * BMAXL;
    const int64_t sa = A.start_a[(int64_t)im * BMAXL + la], sb = A.start_b[(int64_t)im * BMAXL + lb];
    const int64_t nba = ca[2 * la + 1], nbb = cb[2 * lb + 1];
    if (nba <= 0 || nbb <= 0) return;            // a flagged pair keeps the record of k_pair_init
    const bool q_of_a = phase == 0 || phase == 2, t_of_a = phase == 1;
    const int64_t q_n = phase == 0 ? nba : phase == 1 ? nbb : phase == 2 ? ca[2 * la] : cb[2 * lb];
    const int64_t t_n = t_of_a ? nba : nbb;
    const int64_t q_s = q_of_a ? sa : sb, t_s = t_of_a ? sa : sb;
    if (q_s < 0 || t_s < 0 || q_s + q_n > px || t_s + t_n > px) return;                     // (tables of another map: nothing outside the lists is read)
    const uint32_t *qlist = (q_of_a ? A.list_a : A.list_b) + S.off[im] + q_s;
    const uint32_t *tlist = (t_of_a ? A.list_a : A.list_b) + S.off[im] + t_s;
    const int64_t q0 = (int64_t)chunk * DCHUNK;
    if (q0 >= q_n) return;
    int qr[DQ], qc[DQ], m[DQ];
#pragma unroll
    for (int j = 0; j < DQ; j++) {
        const int64_t idx = q0 + j * MTPB + tid;
        const uint32_t v = idx < q_n ? qlist[idx] : 0u;
        qr[j] = (int)(v >> 16); qc[j] = (int)(v & 0xffffu); m[j] = INT_MAX;
    }
    for (int64_t t0 = 0; t0 < t_n; t0 += DTILE) {
        const int nt = t_n - t0 < DTILE ? (int)(t_n - t0) : DTILE;
        __syncthreads();
        for (int k = tid; k < nt; k += MTPB) {
            const uint32_t v = tlist[t0 + k];
            tile[k] = make_int2((int)(v >> 16), (int)(v & 0xffffu));
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < nt; k++) {
            const int2 t = tile[k];
#pragma unroll
            for (int j = 0; j < DQ; j++) {
                const int dr = qr[j] - t.x, dc = qc[j] - t.y;
                const int d = __mul24(dr, dr) + __mul24(dc, dc);
                m[j] = d < m[j] ? d : m[j];
            }
        }
    }
    int32_t mx = -1;
    u64 s1 = 0, s2 = 0;                          // phases 0, 1: the sum of q; phases 2, 3: numerator and denominator
    const int32_t *other = (phase == 2 ? A.b : A.a) + S.off[im];
    const int32_t other_label = phase == 2 ? lb : la;
#pragma unroll
    for (int j = 0; j < DQ; j++) {
        if (q0 + j * MTPB + tid >= q_n) continue;
        const u64 q = quantised_distance(m[j]);
        if (phase < 2) {
            mx = m[j] > mx ? m[j] : mx;
            s1 += q;
        } else {
            const bool both = qr[j] < H && qc[j] < W && other[(int64_t)qr[j] * W + qc[j]] == other_label;
            if (phase == 2) { s2 += q; if (!both) s1 += q; }
            else if (!both) { s1 += q; s2 += q; }            // (a pixel of both objects was visited in phase 2)
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t tm = __shfl_down(mx, o);
        mx = tm > mx ? tm : mx;
        s1 += __shfl_down(s1, o);
        s2 += __shfl_down(s2, o);
    }
    if ((tid & 63) == 0) { redm[tid >> 6] = mx; red1[tid >> 6] = s1; red2[tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < MTPB / 64; k++) { mx = redm[k] > mx ? redm[k] : mx; s1 += red1[k]; s2 += red2[k]; }
        sdsm_pair_distance *R = recs + pair;
        if (phase == 0) { atomicMax(&R->max_d2_ab, mx); atomicAdd((u64 *)&R->sum_q_ab, s1); }
        else if (phase == 1) { atomicMax(&R->max_d2_ba, mx); atomicAdd((u64 *)&R->sum_q_ba, s1); }
        else { if (s1) atomicAdd((u64 *)&R->nsd_num, s1); if (s2) atomicAdd((u64 *)&R->nsd_den, s2); }
    }
}

}  // namespace

extern "C" hipError_t sdsm_label_pixel_counts_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, int32_t *counts, int32_t *bad,
                                                   hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_images * 2 * BMAXL * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, (size_t)n_images * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    grid_pixels(S, LBAND);
    hipLaunchKernelGGL(k_label_pixel_counts, dim3(S.start[n_images]), dim3(MTPB), 0, stream, S, labels, counts, bad);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_label_pixel_lists_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int32_t *counts,
                                                  int32_t *start, int32_t *cursor, uint32_t *list, hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    hipLaunchKernelGGL(k_label_starts, dim3(n_images), dim3(MTPB), 0, stream, counts, start, cursor);
    grid_pixels(S, LBAND);
    hipLaunchKernelGGL(k_label_pixel_lists, dim3(S.start[n_images]), dim3(MTPB), 0, stream, S, labels, counts, start, cursor, list);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_pair_distances_impl(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b,
                                               const int32_t *counts_a, const int32_t *counts_b, const int32_t *start_a, const int32_t *start_b,
                                               const uint32_t *list_a, const uint32_t *list_b, int n_pairs, const int32_t *pairs, int64_t n_items,
                                               const int32_t *items, sdsm_pair_distance *recs, hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    const DArgs A = {d_a, d_b, counts_a, counts_b, start_a, start_b, list_a, list_b};
    hipLaunchKernelGGL(k_pair_init, dim3((n_pairs + MTPB - 1) / MTPB), dim3(MTPB), 0, stream, S, A, n_pairs, pairs, recs);
    if (n_items > 0) hipLaunchKernelGGL(k_pair_distances, dim3((unsigned)n_items), dim3(MTPB), 0, stream, S, A, n_pairs, pairs, items, recs);
    return hipGetLastError();
}

extern "C" void sdsm_quantised_distance_impl(const int32_t *d2, int64_t n, int64_t *out)
{
    for (int64_t k = 0; k < n; k++) out[k] = (int64_t)quantised_distance(d2[k]);
}

// the scale step alone, for the tables that quantise intensities as these do (sdsm_depth.hip)
extern "C" hipError_t sdsm_measure_scale_impl(const sdsm_set_image *images, int n_images, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                              hipStream_t stream)
{
    return launch_scale(make_set(images, n_images), d_g, d_gmax_abs, d_scale_exp, stream);
}

extern "C" hipError_t sdsm_measure_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                const int64_t *bits_off, const uint32_t *bits, const double *d_g, double *d_gmax_abs,
                                                int32_t *d_scale_exp, sdsm_measure_record *out, hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    hipError_t e = launch_scale(S, d_g, d_gmax_abs, d_scale_exp, stream);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(k_measure_objects, dim3(n), dim3(MTPB), 0, stream, S, obj_image, boxes, bits_off, bits, d_g, (const u64 *)d_gmax_abs, out);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_measure_labels_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int64_t *rec_off,
                                               const int32_t *n_labels, const double *d_g, double *d_gmax_abs, int32_t *d_scale_exp,
                                               sdsm_measure_record *out, int32_t *bad, hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    for (int i = 0; i < n_images; i++) { S.rec_off[i] = rec_off[i]; S.n_labels[i] = n_labels[i]; }
    hipError_t e = launch_scale(S, d_g, d_gmax_abs, d_scale_exp, stream);
    if (e != hipSuccess) return e;
    SetLabels R = S;
    grid_records(R);
    hipLaunchKernelGGL(k_labels_init, dim3(R.start[n_images]), dim3(MTPB), 0, stream, R, out, bad);
    grid_pixels(S, LBAND);
    hipLaunchKernelGGL(k_measure_labels, dim3(S.start[n_images]), dim3(MTPB), 0, stream, S, labels, d_g, (const u64 *)d_gmax_abs, out, bad);
    hipLaunchKernelGGL(k_labels_finish, dim3(R.start[n_images]), dim3(MTPB), 0, stream, R, out, d_g ? (const u64 *)d_gmax_abs : nullptr);
    return hipGetLastError();
}

// The tables are cleared here, on the stream: keys to PAIR_FREE (bytes 0xFF), counts and status to 0; slots of images that follow each
// other in the buffers are cleared by one call.
extern "C" hipError_t sdsm_overlap_pairs_impl(const sdsm_set_image *images, int n_images, const int32_t *d_a, const int32_t *d_b,
                                              const int64_t *table_off, const int64_t *capacity, uint64_t *d_keys, uint64_t *d_counts,
                                              int32_t *d_status, hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    OCap C{};
    for (int i = 0; i < n_images; i++) { S.rec_off[i] = table_off[i]; C.cap[i] = capacity[i]; }
    for (int i = 0; i < n_images;) {
        int j = i + 1;
        while (j < n_images && table_off[j] == table_off[j - 1] + capacity[j - 1]) j++;
        const size_t first = (size_t)table_off[i], bytes = (size_t)(table_off[j - 1] + capacity[j - 1] - table_off[i]) * sizeof(u64);
        hipError_t e = hipMemsetAsync(d_keys + first, 0xFF, bytes, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_counts + first, 0, bytes, stream);
        if (e != hipSuccess) return e;
        i = j;
    }
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_images * 2 * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    grid_pixels(S, LBAND);
    hipLaunchKernelGGL(k_overlap_pairs, dim3(S.start[n_images]), dim3(MTPB), 0, stream, S, C, d_a, d_b, (u64 *)d_keys, (u64 *)d_counts, d_status);
    return hipGetLastError();
}
