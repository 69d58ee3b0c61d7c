// Depth tables on the GPU: one sdsm_depth_record and n_shells sdsm_depth_shell_record per object (bit-packed fragments) or per label (the
// windows of sdsm_shape.hip), for one image or a set of images.  No reference counterpart; the definition the kernel is tested against is
// the host code of superdsm_amd/depth.py.
//
//   k_depth_objects   one workgroup of 256 threads per fragment: an exact squared Euclidean distance transform of the fragment alone --
//                     everything that is not a set bit of it is outside, the places one step beyond its box included -- and the
//                     reductions over it.
//     column pass   a thread per column of the box: g(r, c), the distance along the column to the nearest place that is clear or outside
//                   the box, as the smaller of a downward and an upward running count (0 for a clear pixel)
//     row pass      a thread per pixel, consecutive lanes on consecutive pixels: d2 = min over c' of (c - c')^2 + g(r, c')^2, scanned
//                   outwards from c while delta^2 < best.  The start value min(g^2, (c + 1)^2, (w - c)^2) already holds the columns beyond
//                   the box, so the scan never leaves the row.  In the same loop the integer sums in registers, the 64-bit key of the
//                   inscribed-circle pixel, and the shell sums by LDS integer adds.
//     n_max         one pass over d2
//     median        an exact radix select over d2, 8-bit digits from the highest byte that max_d2 has (one or two rounds for every
//                   object that fits LDS); the rank above is the same value or, by one more pass, the smallest value above it
//   A box of at most SDSM_DEPTH_LDS_PIXELS pixels keeps its bits, g and d2 (uint16 each) in LDS; a larger one runs the same code over
//   the caller's workspace (uint32 each) and reads its bits from global memory: the same bytes, more slowly.
// No global atomics, no float atomics, no output that needs clearing.
#include "sdsm_tables.h"
#include "sdsm_quantile.h"
#include "sdsm_depth.h"
#include <climits>

static_assert(SDSM_DEPTH_MAX_SHELLS == SDSM_DEPTH_MAX_SHELLS_INLINE, "the limit of the header and of the inline helper");
static_assert(sizeof(sdsm_depth_record) == 80 && sizeof(sdsm_depth_shell_record) == 32, "the sizes of include/sdsm.h and of _capi.py");

namespace {

constexpr int DTPB = 256;                        // threads of a workgroup = bins of a histogram
constexpr int DWAVES = DTPB / 64;
constexpr int LPIX = SDSM_DEPTH_LDS_PIXELS;
constexpr int NS = SDSM_DEPTH_MAX_SHELLS;
static_assert(LPIX % 32 == 0 && LPIX <= 65536, "whole words; g <= h / 2 + 1 and d2 <= (min(h, w) / 2 + 1)^2 of a box in LDS fit uint16");

struct DLds {                                    // 53 KB: three workgroups per compute unit
    uint16_t g[LPIX], d2[LPIX];
    uint32_t words[LPIX / 32];
    uint32_t hist[DTPB];
    u64 sh_count[NS], sh_finite[NS], sh_lo[NS], sh_hi[NS];
    u64 r64[DWAVES][4];
    int32_t r32[DWAVES][6];
    uint32_t sel_bin, sel_r, sel_cnt;
};

__device__ __forceinline__ void zero_result(sdsm_depth_record *out, sdsm_depth_shell_record *sh, int n_shells, int tid, int flags)
{
    if (tid == 0) {
        sdsm_depth_record R;
        R.area = R.max_d2 = 0; R.max_row = R.max_col = 0; R.n_max = R.sum_d2 = R.sum_q = R.med_d2_lo = R.med_d2_hi = R.n_rim = 0;
        R.flags = flags; R.scale_exp = 0;
        *out = R;
    }
    if (tid < n_shells) {
        sdsm_depth_shell_record Z;
        Z.count = Z.n_finite = 0; Z.gsum_lo = 0; Z.gsum_hi = 0;
        sh[tid] = Z;
    }
}

// The value at rank r (from 0) of the non-zero entries of D; below: entries smaller than it, eq: entries equal to it.  r is the same in
// every thread and smaller than the number of non-zero entries, none of which has a bit above the byte at `top`.
template <class T>
__device__ __forceinline__ uint32_t radix_select(const T *D, uint32_t npx, DLds &L, int tid, uint32_t r, int top, uint32_t &below, uint32_t &eq)
{
    uint32_t prefix = 0;
    const uint32_t rank = r;
    for (int shift = top; shift >= 0; shift -= 8) {
        L.hist[tid] = 0;
        __syncthreads();
        const uint32_t above = shift == 24 ? 0u : ~0u << (shift + 8);             // the digits already fixed
        for (uint32_t p = tid; p < npx; p += DTPB) {
            const uint32_t k = D[p];
            if (k && (k & above) == prefix) atomicAdd(&L.hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) select_bin(L.hist, tid, r, L.sel_bin, L.sel_r, L.sel_cnt);     // one wavefront
        __syncthreads();
        prefix |= L.sel_bin << shift;
        r = L.sel_r;
        eq = L.sel_cnt;
    }
    below = rank - r;
    return prefix;
}

// x summed (ADD) or its maximum taken over the workgroup; every thread receives the result
template <bool ADD>
__device__ __forceinline__ u64 block_reduce(DLds &L, int tid, u64 x)
{
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_down(x, o);
        x = ADD ? x + t : (t > x ? t : x);
    }
    __syncthreads();                             // (r64 may still be read from the reduction before)
    if ((tid & 63) == 0) L.r64[tid >> 6][0] = x;
    __syncthreads();
    x = L.r64[0][0];
    for (int k = 1; k < DWAVES; k++) x = ADD ? x + L.r64[k][0] : (L.r64[k][0] > x ? L.r64[k][0] : x);
    return x;
}

// The object of fragment f with its bits at wb, its column distances in G and its squared depths in D (h * w entries each, LDS or the
// caller's workspace).  g: the image's intensities or null, e: its scale exponent.
template <class T>
__device__ __forceinline__ void depth_object(DLds &L, T *G, T *D, const uint32_t *wb, const Fragment &f, const double *g, int e, int n_shells, int tid,
                                             sdsm_depth_record *out, sdsm_depth_shell_record *sh)
{
    const int h = f.h, w = f.w;
    const uint32_t npx = (uint32_t)h * (uint32_t)w;
    if (tid < NS) L.sh_count[tid] = L.sh_finite[tid] = L.sh_lo[tid] = L.sh_hi[tid] = 0;

    // ---- column pass ---------------------------------------------------------------------------------------------------------------
    for (int c = tid; c < w; c += DTPB) {
        uint32_t run = 0, p = (uint32_t)c;
        for (int r = 0; r < h; r++, p += (uint32_t)w) {
            run = ((wb[p >> 5] >> (p & 31)) & 1u) ? run + 1 : 0;                  // (p < h * w: a bit past the fragment is never read as a pixel)
            G[p] = (T)run;
        }
        run = 0;
        for (int r = h - 1; r >= 0; r--) {
            p -= (uint32_t)w;
            run = ((wb[p >> 5] >> (p & 31)) & 1u) ? run + 1 : 0;
            if (run < (uint32_t)G[p]) G[p] = (T)run;
        }
    }
    __syncthreads();

    // ---- row pass, sums, shells --------------------------------------------------------------------------------------------------------
    uint32_t area = 0, n_rim = 0;
    u64 sum_d2 = 0, sum_q = 0, key = 0;
    int rmin = INT_MAX, cmin = INT_MAX, rmax = -1, cmax = -1;
    const int dr = DTPB / w, dc = DTPB % w;
    int r = tid / w, c = tid % w;
    for (uint32_t p = tid; p < npx; p += DTPB) {
        const uint32_t gv = G[p];
        uint32_t best = 0;
        if (gv) {
            const uint32_t m = (uint32_t)(c + 1 < w - c ? c + 1 : w - c);         // columns to the nearest place beyond the box
            best = gv * gv;                      // (gv, m <= 32 768: the squares and their sums stay below 2^31)
            best = m * m < best ? m * m : best;
            const T *row = G + (p - (uint32_t)c);
            for (uint32_t d = 1; d * d < best; d++) {                             // d < m: c - d and c + d are columns of the box
                const uint32_t a = row[c - (int)d], b = row[c + (int)d];
                const uint32_t va = a * a + d * d, vb = b * b + d * d;
                best = va < best ? va : best;
                best = vb < best ? vb : best;
            }
            area++;
            n_rim += best == 1 ? 1 : 0;
            sum_d2 += best;
            sum_q += quantised_distance((int32_t)best);
            const u64 k = ((u64)best << 32) | (u64)(0xffffffffu - p);
            key = k > key ? k : key;
            rmin = r < rmin ? r : rmin; rmax = r > rmax ? r : rmax;
            cmin = c < cmin ? c : cmin; cmax = c > cmax ? c : cmax;
            const int s = sdsm_depth_shell_inline((int32_t)best, n_shells);
            atomicAdd(&L.sh_count[s], 1ull);
            if (g) {
                const double v = g[(int64_t)(f.r0 + r) * f.W + f.c0 + c];
                if (finite_bits(v)) {
                    const i64 q = (i64)rint(ldexp(v, 62 - e));                   // |q| <= 2^62
                    atomicAdd(&L.sh_finite[s], 1ull);
                    atomicAdd(&L.sh_lo[s], (u64)(uint32_t)q);
                    atomicAdd(&L.sh_hi[s], (u64)(q >> 32));
                }
            }
        }
        D[p] = (T)best;
        r += dr; c += dc;
        if (c >= w) { c -= w; r++; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_down(area, o); n_rim += __shfl_down(n_rim, o); sum_d2 += __shfl_down(sum_d2, o); sum_q += __shfl_down(sum_q, o);
        const u64 k = __shfl_down(key, o);
        key = k > key ? k : key;
        const int t0 = __shfl_down(rmin, o), t1 = __shfl_down(cmin, o), t2 = __shfl_down(rmax, o), t3 = __shfl_down(cmax, o);
        rmin = t0 < rmin ? t0 : rmin; cmin = t1 < cmin ? t1 : cmin; rmax = t2 > rmax ? t2 : rmax; cmax = t3 > cmax ? t3 : cmax;
    }
    if ((tid & 63) == 0) {
        const int wv = tid >> 6;
        L.r64[wv][0] = ((u64)n_rim << 32) | area; L.r64[wv][1] = sum_d2; L.r64[wv][2] = sum_q; L.r64[wv][3] = key;
        L.r32[wv][0] = rmin; L.r32[wv][1] = cmin; L.r32[wv][2] = rmax; L.r32[wv][3] = cmax;
    }
    __syncthreads();                             // (and D and the shell sums are complete)
    i64 n_area = 0, rim = 0;
    sum_d2 = sum_q = key = 0; rmin = cmin = INT_MAX; rmax = cmax = -1;
    for (int k = 0; k < DWAVES; k++) {           // every thread: the same values
        n_area += (i64)(L.r64[k][0] & 0xffffffffull); rim += (i64)(L.r64[k][0] >> 32);
        sum_d2 += L.r64[k][1]; sum_q += L.r64[k][2];
        key = L.r64[k][3] > key ? L.r64[k][3] : key;
        rmin = L.r32[k][0] < rmin ? L.r32[k][0] : rmin; cmin = L.r32[k][1] < cmin ? L.r32[k][1] : cmin;
        rmax = L.r32[k][2] > rmax ? L.r32[k][2] : rmax; cmax = L.r32[k][3] > cmax ? L.r32[k][3] : cmax;
    }
    if (n_area == 0) {                           // (uniform)
        zero_result(out, sh, n_shells, tid, 0);
        return;
    }
    const uint32_t max_d2 = (uint32_t)(key >> 32), p_max = 0xffffffffu - (uint32_t)key;

    // ---- the pixels at the maximum ---------------------------------------------------------------------------------------------------------
    u64 n_max = 0;
    for (uint32_t p = tid; p < npx; p += DTPB) n_max += (uint32_t)D[p] == max_d2 ? 1 : 0;
    n_max = block_reduce<true>(L, tid, n_max);

    // ---- the median ------------------------------------------------------------------------------------------------------------------------
    int64_t lo, hi, rem;
    sdsm_quantile_ranks_inline(n_area, 1, 2, &lo, &hi, &rem);
    const int top = max_d2 < (1u << 8) ? 0 : max_d2 < (1u << 16) ? 8 : max_d2 < (1u << 24) ? 16 : 24;
    uint32_t below, eq;
    const uint32_t k_lo = radix_select(D, npx, L, tid, (uint32_t)lo, top, below, eq);
    uint32_t k_hi = k_lo;
    if (hi != lo && (uint32_t)lo - below + 1 >= eq) {                             // rank lo is the last of its equals: the smallest value above
        u64 m = 0;                               // (as the maximum of the complement)
        for (uint32_t p = tid; p < npx; p += DTPB) {
            const uint32_t k = D[p];
            if (k > k_lo && (u64)(0xffffffffu - k) > m) m = 0xffffffffu - k;
        }
        k_hi = 0xffffffffu - (uint32_t)block_reduce<false>(L, tid, m);
    }

    if (tid == 0) {
        sdsm_depth_record R;
        R.area = n_area; R.max_d2 = max_d2;
        R.max_row = f.r0 + (int)(p_max / (uint32_t)w); R.max_col = f.c0 + (int)(p_max % (uint32_t)w);
        R.n_max = (i64)n_max; R.sum_d2 = (i64)sum_d2; R.sum_q = (i64)sum_q; R.med_d2_lo = k_lo; R.med_d2_hi = k_hi; R.n_rim = rim;
        R.flags = (f.r0 + rmin == 0 || f.c0 + cmin == 0 || f.r0 + rmax + 1 == f.H || f.c0 + cmax + 1 == f.W) ? 1 : 0;
        R.scale_exp = e;
        *out = R;
    }
    if (tid < n_shells) {
        sdsm_depth_shell_record Z;
        Z.count = (i64)L.sh_count[tid]; Z.n_finite = (i64)L.sh_finite[tid]; Z.gsum_lo = L.sh_lo[tid]; Z.gsum_hi = (i64)L.sh_hi[tid];
        sh[tid] = Z;
    }
}

__global__ __launch_bounds__(DTPB) void k_depth_objects(SetImages S, const int32_t *obj_image, const int32_t *boxes, const int64_t *bits_off,
                                                        const uint32_t *bits_, const double *g_, const u64 *maxbits, int n_shells, const int64_t *ws_off,
                                                        uint32_t *ws, int64_t ws_pixels, sdsm_depth_record *out, sdsm_depth_shell_record *shells)
{
    __shared__ DLds L;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int im = obj_image ? obj_image[i] : 0;
    sdsm_depth_shell_record *sh = shells + (int64_t)i * n_shells;
    Fragment f;
    if (!fragment_box(S, im, boxes, i, f)) {     // (uniform: the whole workgroup leaves; nothing is read)
        zero_result(out + i, sh, n_shells, tid, 0);
        return;
    }
    const int64_t npx = (int64_t)f.h * f.w;
    const uint32_t *bits = bits_ + bits_off[i];
    const double *g = g_ ? g_ + S.off[im] : nullptr;
    const int e = g_ ? scale_exp(maxbits[im]) : 0;
    if (npx <= LPIX) {
        const uint32_t n_words = ((uint32_t)npx + 31) >> 5;
        for (uint32_t k = tid; k < n_words; k += DTPB) L.words[k] = bits[k];
        __syncthreads();
        depth_object<uint16_t>(L, L.g, L.d2, L.words, f, g, e, n_shells, tid, out + i, sh);
    } else {
        const int64_t off = ws_off ? ws_off[i] : -1;
        if (!ws || off < 0 || off > ws_pixels - npx) {                            // no room named for this box: flagged, nothing is written there
            zero_result(out + i, sh, n_shells, tid, SDSM_DEPTH_NO_WORKSPACE);
            return;
        }
        uint32_t *G = ws + 2 * off;
        depth_object<uint32_t>(L, G, G + npx, bits, f, g, e, n_shells, tid, out + i, sh);
    }
}

}  // namespace

extern "C" hipError_t sdsm_depth_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                              const int64_t *bits_off, const uint32_t *bits, const double *d_g, const double *d_gmax_abs, int n_shells,
                                              const int64_t *d_ws_off, void *d_ws, int64_t ws_pixels, sdsm_depth_record *out,
                                              sdsm_depth_shell_record *shells, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const SetImages S = make_set(images, n_images);
    hipLaunchKernelGGL(k_depth_objects, dim3(n), dim3(DTPB), 0, stream, S, obj_image, boxes, bits_off, bits, d_g, (const u64 *)d_gmax_abs, n_shells, d_ws_off,
                       (uint32_t *)d_ws, ws_pixels, out, shells);
    return hipGetLastError();
}
