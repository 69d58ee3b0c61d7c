// Texture tables on the GPU: per object (bit-packed fragments, or the label windows of sdsm_shape.hip) and offset the non-zero cells of
// the grey-level co-occurrence matrix, for one image or a set of images.  No reference counterpart; the definition the kernels are tested
// against is the host code of superdsm_amd/texture.py.
//
//   k_texture          one workgroup of 256 threads per (object, offset).  Dynamic LDS sized by the levels G: the G - 1 edges of the
//                      object's image, then the packed upper triangle of the counts, G (G + 1) / 2 uint32 (131 584 B at G = 256: one
//                      workgroup per compute unit there).
//     clear            the triangle
//     pairs            the fragment's words are walked by ctz (as k_intensity_objects).  The neighbours of the 32 pixels of a word are
//                      the 32 bits from bit 32 k + d_row w + d_col of the fragment on -- two words, shifted; bits before the first and
//                      past the h w-th are 0, so a neighbour row outside the box reads 0 --, and a neighbour whose column leaves
//                      0 .. w - 1 (it wrapped into the next row) is dropped.  Levels by binary search over the edges in LDS, found on the
//                      fly: one search per pixel, one more per pair.  A pair is one LDS integer add whose result is not used.
//     compaction       thread t owns the cells t s .. t s + s - 1 (s odd: neighbouring threads start on different banks); it counts its
//                      non-zero cells, one workgroup-wide exclusive scan gives its place, and it writes them in cell order.  The order of
//                      the entries therefore does not depend on scheduling.
//   k_texture_scan     `first`: the exclusive sum of n_entries over all (object, offset), one workgroup
//   k_texture_gather   the padded lists one behind the other
// The record of an object (area, finite pixels, level range, flags) is found by every workgroup of the object on its way and written by
// that of offset 0.  The only floating-point operations are comparisons; no float atomics, no global atomics, no output needs clearing.
#include "sdsm_tables.h"
#include "sdsm_texture.h"
#include <climits>

namespace {

constexpr int TTPB = 256;
constexpr int TWAVES = TTPB / 64;

struct TOffsets {                                // the offsets of a launch
    int32_t n;
    int32_t dr[SDSM_TEXTURE_MAX_OFFSETS], dc[SDSM_TEXTURE_MAX_OFFSETS];
};

struct TRed {
    u64 r64[TWAVES][3];
    int32_t r32[TWAVES][7];
    uint32_t scan[TWAVES];
};

// word q of the fragment; 0 outside it, and the bits past h * w are not the object's
__device__ __forceinline__ uint32_t word_at(const uint32_t *bits, i64 q, uint32_t n_words, uint32_t n_bits)
{
    if (q < 0 || q >= (i64)n_words) return 0;
    uint32_t w = bits[q];
    if (q == (i64)n_words - 1 && (n_bits & 31)) w &= (1u << (n_bits & 31)) - 1;
    return w;
}

// the 32 bits of the fragment from bit p on (p may be negative or past the end)
__device__ __forceinline__ uint32_t bits_from(const uint32_t *bits, i64 p, uint32_t n_words, uint32_t n_bits)
{
    const i64 q = p >> 5;                        // (arithmetic shift: the floor)
    const int s = (int)(p & 31);
    const uint32_t lo = word_at(bits, q, n_words, n_bits);
    if (s == 0) return lo;
    return (lo >> s) | (word_at(bits, q + 1, n_words, n_bits) << (32 - s));
}

__device__ __forceinline__ void empty_result(sdsm_texture_record *out, sdsm_texture_pairs *P, bool record, int levels, i64 area, int flags)
{
    if (record) {
        sdsm_texture_record R;
        R.area = area; R.n_finite = 0; R.level_min = levels; R.level_max = -1; R.flags = flags | 4; R.reserved = 0;
        *out = R;
    }
    P->n_pairs = 0; P->n_entries = 0; P->reserved = 0;                              // (`first` is k_texture_scan's)
}

__global__ __launch_bounds__(TTPB) void k_texture(SetImages S, TOffsets O, int levels, const double *edges_, const int32_t *obj_image, const int32_t *boxes,
                                                  const int64_t *bits_off, const uint32_t *bits_, const double *g_, const int64_t *slot_off,
                                                  sdsm_texture_entry *slots, sdsm_texture_record *out, sdsm_texture_pairs *pairs)
{
    extern __shared__ __align__(8) unsigned char t_dyn[];
    __shared__ TRed T;
    const int n_edges = levels - 1, n_cells = levels * (levels + 1) / 2;
    double *edges = (double *)t_dyn;
    uint32_t *tri = (uint32_t *)(t_dyn + 8 * (size_t)n_edges);
    const int i = blockIdx.x, o = blockIdx.y, tid = threadIdx.x;
    sdsm_texture_pairs *P = pairs + ((int64_t)i * O.n + o);
    const int im = obj_image ? obj_image[i] : 0;
    // (fragment_box and each_set_bit of sdsm_tables.h, written out: see "What the table kernels share" in DESIGN.md)
    const bool im_ok = im >= 0 && im < S.n;
    const int H = im_ok ? S.H[im] : 0, W = im_ok ? S.W[im] : 0;
    const int br0 = boxes[4 * i], bc0 = boxes[4 * i + 1], h = boxes[4 * i + 2], w = boxes[4 * i + 3];
    if (!(im_ok && br0 >= 0 && bc0 >= 0 && h >= 1 && w >= 1 && h <= H && w <= W && br0 <= H - h && bc0 <= W - w)) {
        if (tid == 0) empty_result(out + i, P, o == 0, levels, 0, 0);              // (uniform: the whole workgroup leaves; nothing is read)
        return;
    }
    const uint32_t *bits = bits_ + bits_off[i];
    const double *g = g_ + S.off[im];
    const uint32_t n_bits = (uint32_t)h * (uint32_t)w, n_words = (n_bits + 31) >> 5;
    for (int e = tid; e < n_edges; e += TTPB) edges[e] = edges_[(int64_t)im * n_edges + e];
    for (int c = tid; c < n_cells; c += TTPB) tri[c] = 0;
    __syncthreads();

    // ---- pairs ---------------------------------------------------------------------------------------------------------------------
    const int dr = O.dr[o], dc = O.dc[o];
    const i64 delta = (i64)dr * w + dc;
    uint32_t area = 0, nfin = 0, npairs = 0;
    int flags = 0, r0 = INT_MAX, c0 = INT_MAX, r1 = 0, c1 = 0, lmin = levels, lmax = -1;
    for (uint32_t k = tid; k < n_words; k += TTPB) {
        uint32_t word = word_at(bits, k, n_words, n_bits);
        if (!word) continue;
        const uint32_t nb = bits_from(bits, ((i64)k << 5) + delta, n_words, n_bits);
        while (word) {
            const int t = __builtin_ctz(word);
            word &= word - 1;
            const uint32_t b = (k << 5) + (uint32_t)t;
            const int cl = (int)(b % (uint32_t)w);
            const int r = br0 + (int)(b / (uint32_t)w), c = bc0 + cl;
            area++;
            r0 = r < r0 ? r : r0; r1 = r + 1 > r1 ? r + 1 : r1;
            c0 = c < c0 ? c : c0; c1 = c + 1 > c1 ? c + 1 : c1;
            const double gp = g[(int64_t)r * W + c];
            if (!finite_bits(gp)) { flags |= 2; continue; }
            nfin++;
            const int a = sdsm_texture_level_inline(edges, n_edges, gp);
            lmin = a < lmin ? a : lmin; lmax = a > lmax ? a : lmax;
            if (!((nb >> t) & 1u) || cl + dc < 0 || cl + dc >= w) continue;      // the neighbour is not in the object, or its column wrapped
            const double gq = g[(int64_t)(r + dr) * W + (c + dc)];                 // (inside the box: its bit is set)
            if (!finite_bits(gq)) continue;
            const int q = sdsm_texture_level_inline(edges, n_edges, gq);
            atomicAdd(&tri[sdsm_texture_cell_inline(levels, a < q ? a : q, a < q ? q : a)], 1u);
            npairs++;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        area += __shfl_down(area, s); nfin += __shfl_down(nfin, s); npairs += __shfl_down(npairs, s); flags |= __shfl_down(flags, s);
        const int t0 = __shfl_down(r0, s), t1 = __shfl_down(c0, s), t2 = __shfl_down(r1, s), t3 = __shfl_down(c1, s);
        const int t4 = __shfl_down(lmin, s), t5 = __shfl_down(lmax, s);
        r0 = t0 < r0 ? t0 : r0; c0 = t1 < c0 ? t1 : c0; r1 = t2 > r1 ? t2 : r1; c1 = t3 > c1 ? t3 : c1;
        lmin = t4 < lmin ? t4 : lmin; lmax = t5 > lmax ? t5 : lmax;
    }
    if ((tid & 63) == 0) {
        const int wv = tid >> 6;
        T.r64[wv][0] = area; T.r64[wv][1] = nfin; T.r64[wv][2] = npairs;
        T.r32[wv][0] = flags; T.r32[wv][1] = r0; T.r32[wv][2] = c0; T.r32[wv][3] = r1; T.r32[wv][4] = c1; T.r32[wv][5] = lmin; T.r32[wv][6] = lmax;
    }
    __syncthreads();                             // (the adds to the triangle are done as well)
    i64 n_area = 0, n = 0, n_pairs = 0;
    flags = 0; r0 = c0 = INT_MAX; r1 = c1 = 0; lmin = levels; lmax = -1;
    for (int k = 0; k < TWAVES; k++) {           // every thread: the same values
        n_area += (i64)T.r64[k][0]; n += (i64)T.r64[k][1]; n_pairs += (i64)T.r64[k][2];
        flags |= T.r32[k][0];
        r0 = T.r32[k][1] < r0 ? T.r32[k][1] : r0; c0 = T.r32[k][2] < c0 ? T.r32[k][2] : c0;
        r1 = T.r32[k][3] > r1 ? T.r32[k][3] : r1; c1 = T.r32[k][4] > c1 ? T.r32[k][4] : c1;
        lmin = T.r32[k][5] < lmin ? T.r32[k][5] : lmin; lmax = T.r32[k][6] > lmax ? T.r32[k][6] : lmax;
    }
    if (n_area > 0 && (r0 == 0 || c0 == 0 || r1 == H || c1 == W)) flags |= 1;
    if (n == 0) flags |= 4;
    if (tid == 0 && o == 0) {
        sdsm_texture_record R;
        R.area = n_area; R.n_finite = n; R.level_min = lmin; R.level_max = lmax; R.flags = flags; R.reserved = 0;
        out[i] = R;
    }

    // ---- compaction in cell order ----------------------------------------------------------------------------------------------------
    const int seg = ((n_cells + TTPB - 1) / TTPB) | 1;
    const int c_lo = tid * seg < n_cells ? tid * seg : n_cells, c_hi = c_lo + seg < n_cells ? c_lo + seg : n_cells;
    uint32_t nz = 0;
    for (int c = c_lo; c < c_hi; c++) nz += tri[c] != 0 ? 1u : 0u;
    uint32_t incl = nz;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(incl, s);
        if ((tid & 63) >= s) incl += t;
    }
    if ((tid & 63) == 63) T.scan[tid >> 6] = incl;
    __syncthreads();
    uint32_t pos = incl - nz, total = 0;
    for (int k = 0; k < TWAVES; k++) {
        if (k < (tid >> 6)) pos += T.scan[k];
        total += T.scan[k];
    }
    const int64_t slot0 = slot_off[(int64_t)i * O.n + o];
    const int64_t cap = slot_off[(int64_t)i * O.n + o + 1] - slot0;
    if (nz) {
        int ci = 0, rem = c_lo;
        while (rem >= levels - ci) { rem -= levels - ci; ci++; }
        int cj = ci + rem;
        for (int c = c_lo; c < c_hi; c++) {
            const uint32_t cnt = tri[c];
            if (cnt) {
                if ((int64_t)pos < cap) {        // (never false for a list of min(h w, cells) entries: cells <= pairs <= pixels)
                    sdsm_texture_entry E;
                    E.i = (uint16_t)ci; E.j = (uint16_t)cj; E.count = cnt;
                    slots[slot0 + pos] = E;
                }
                pos++;
            }
            if (++cj == levels) { ci++; cj = ci; }
        }
    }
    if (tid == 0) {
        const int64_t room = cap > 0 ? cap : 0;
        P->n_pairs = n_pairs; P->n_entries = (int32_t)((int64_t)total < room ? (int64_t)total : room); P->reserved = 0;
    }
}

// pairs[m].first: the exclusive sum of n_entries.  One workgroup walks the list 256 at a time.
__global__ __launch_bounds__(TTPB) void k_texture_scan(int64_t m, sdsm_texture_pairs *pairs)
{
    __shared__ i64 wsum[TWAVES];
    const int tid = threadIdx.x;
    i64 running = 0;
    for (int64_t base = 0; base < m; base += TTPB) {
        const int64_t idx = base + tid;
        const i64 v = idx < m ? (i64)pairs[idx].n_entries : 0;
        i64 incl = v;
        for (int s = 1; s < 64; s <<= 1) {
            const i64 t = __shfl_up(incl, s);
            if ((tid & 63) >= s) incl += t;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        i64 before = 0, all = 0;
        for (int k = 0; k < TWAVES; k++) {
            if (k < (tid >> 6)) before += wsum[k];
            all += wsum[k];
        }
        if (idx < m) pairs[idx].first = running + before + incl - v;
        running += all;
        __syncthreads();                         // (wsum is written again in the next round)
    }
}

__global__ __launch_bounds__(TTPB) void k_texture_gather(const int64_t *slot_off, const sdsm_texture_entry *slots, const sdsm_texture_pairs *pairs,
                                                         sdsm_texture_entry *entries)
{
    const int64_t m = blockIdx.x;
    const sdsm_texture_entry *src = slots + slot_off[m];
    sdsm_texture_entry *dst = entries + pairs[m].first;
    const int n = pairs[m].n_entries;
    for (int k = threadIdx.x; k < n; k += TTPB) dst[k] = src[k];
}

// hipFuncSetAttribute costs microseconds per call: the dynamic LDS limit of k_texture is raised only when a launch needs more than before
// (as need_lds of sdsm_prepare.hip)
hipError_t texture_lds(size_t bytes)
{
    static thread_local size_t seen[64] = {};
    if (bytes <= 32 * 1024) return hipSuccess;   // (every kernel may have that much without asking)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFuncSetAttribute((const void *)k_texture, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (seen[dev] >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)k_texture, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) seen[dev] = bytes;
    return e;
}

}  // namespace

extern "C" hipError_t sdsm_texture_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                const int64_t *bits_off, const uint32_t *bits, const double *d_g, int levels, const double *d_edges,
                                                int n_offsets, const int32_t *offsets, const int64_t *slot_off, sdsm_texture_entry *slots,
                                                sdsm_texture_record *out, sdsm_texture_pairs *pairs, sdsm_texture_entry *entries, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const SetImages S = make_set(images, n_images);
    TOffsets O{};
    O.n = n_offsets;
    for (int o = 0; o < n_offsets; o++) { O.dr[o] = offsets[2 * o]; O.dc[o] = offsets[2 * o + 1]; }
    const size_t lds = 8 * (size_t)(levels - 1) + 4 * (size_t)(levels * (levels + 1) / 2);
    static_assert(8 * (SDSM_TEXTURE_MAX_LEVELS - 1) + 2 * SDSM_TEXTURE_MAX_LEVELS * (SDSM_TEXTURE_MAX_LEVELS + 1) + sizeof(TRed) <= 160 * 1024 - 512, "LDS budget");
    hipError_t e = texture_lds(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_texture, dim3(n, n_offsets), dim3(TTPB), lds, stream, S, O, levels, d_edges, obj_image, boxes, bits_off, bits, d_g, slot_off, slots, out,
                       pairs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t m = (int64_t)n * n_offsets;
    hipLaunchKernelGGL(k_texture_scan, dim3(1), dim3(TTPB), 0, stream, m, pairs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_texture_gather, dim3((unsigned)m), dim3(TTPB), 0, stream, slot_off, slots, pairs, entries);
    return hipGetLastError();
}
