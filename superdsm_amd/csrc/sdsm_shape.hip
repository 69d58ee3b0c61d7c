// Contour shape tables on the GPU: one sdsm_shape_record of exact integers per object (bit-packed fragments) or per label (label maps)
// and the vertices of its convex hull, for one image or a set of images.  No reference counterpart; the definition every kernel is
// tested against is the host code of superdsm_amd/shape.py.
//
//   k_shape_objects   one workgroup per fragment.  The fragment's bits are contiguous over h * w, not row-aligned: they go through LDS
//                     as aligned bit rows P_r (word j of a row = columns 32 j .. 32 j + 31), a window larger than the LDS tile in row
//                     bands with a two-row halo and, beyond 126 words of width, in column tiles with a one-word halo.  Word-wise the
//                     border row is E_r = P_r & ~(P_r-1 & P_r+1 & P_r << 1 & P_r >> 1); the edge counts are popcounts of P_r & ~neighbour,
//                     the perimeter classes popcounts of bit-sliced sums of the eight shifted border rows.  The first and last set bit of
//                     every row (LDS integer min / max) give four corner candidates per occupied row; lane 0 of wave 0 walks the left
//                     chain of the hull and lane 0 of wave 1 the right one (monotone chain, stacks in LDS: a step depends on the one
//                     before), band after band.  Twice the hull area and the largest squared distance of two vertices are computed by
//                     the whole workgroup.  All counts are integer reductions (shuffles, then 64-bit LDS adds).
//   k_shape_offsets / k_shape_gather   the exclusive sum of n_vertices, and the vertices of all objects one behind the other
//   k_shape_scatter   label form: every pixel sets its bit in the window of its label (a thread owns 32 consecutive pixels and issues one
//                     integer atomic or per word and run), after which the windows are fragments like any other
#include "sdsm_tables.h"
#include <climits>

namespace {

constexpr int STPB = 256;
constexpr int PE_WORDS = 1024;                   // LDS words of the tile: the rows of P and of E (4 KB)
constexpr int TWMAX = PE_WORDS / 8 - 2;          // words of a column tile: 5 rows of P and 3 of E with their halo words fit
constexpr int BMAX = 254;                        // rows of a band
constexpr int SL = SDSM_SHAPE_MAX_CHAIN;         // entries of a chain's stack (16 KB each)
constexpr int SSEG = 32;                         // k_shape_scatter: consecutive pixels of a thread
constexpr int SBAND = SSEG * STPB;               //   pixels of a workgroup

struct ShapeLds {
    uint32_t pe[PE_WORDS];
    uint32_t chain_l[SL], chain_r[SL];           // row << 16 | column, window lattice coordinates (both <= 65535)
    int32_t first[BMAX + 2], last[BMAX + 2];     // [0]: the row before the band, [1 .. nb]: its rows, [nb + 1]: empty
    u64 cnt[7];
    u64 area2, d2max;
    int32_t nl, nr, rmin, rmax, cmin, cmax, overflow;
};

// Columns 32 j .. 32 j + 31 of row R of an h x w window whose bits are contiguous from bits[0] on; 0 outside the window.  Bits past
// h * w are never part of a row.
__device__ __forceinline__ uint32_t window_word(const uint32_t *bits, uint32_t n_words, int h, int w, int R, int j)
{
    if (R < 0 || R >= h || j < 0 || j * 32 >= w) return 0;
    const uint32_t s = (uint32_t)R * (uint32_t)w + (uint32_t)j * 32u;        // < h * w < 2^31
    const uint32_t k = s >> 5, sh = s & 31;
    uint32_t v = bits[k] >> sh;
    if (sh && k + 1 < n_words) v |= bits[k + 1] << (32 - sh);
    const int ncol = w - j * 32;
    return ncol < 32 ? v & ((1u << ncol) - 1) : v;
}

// the three bit planes of a + b + c + d, bit by bit
__device__ __forceinline__ void sum4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t &s0, uint32_t &s1, uint32_t &s2)
{
    const uint32_t x = a ^ b, y = c ^ d, ca = a & b, cb = c & d, k = x & y;
    s0 = x ^ y; s1 = ca ^ cb ^ k; s2 = ca & cb;
}

__device__ __forceinline__ i64 cross3(uint32_t o, uint32_t a, int y, int x)
{
    const i64 oy = o >> 16, ox = o & 0xffffu, ay = a >> 16, ax = a & 0xffffu;
    return (ay - oy) * (x - ox) - (ax - ox) * (y - oy);
}

// one step of a chain: the point (y, x) against the stack; the left chain keeps strict left turns (sign +1), the right one right turns
__device__ __forceinline__ void chain_push(uint32_t *st, int &n, int y, int x, int sign, int32_t *overflow)
{
    while (n >= 2 && sign * cross3(st[n - 2], st[n - 1], y, x) <= 0) n--;
    if (n < SL) st[n++] = ((uint32_t)y << 16) | (uint32_t)x;
    else *overflow = 1;
}

__device__ __forceinline__ void zero_record(sdsm_shape_record *out)
{
    sdsm_shape_record R;
    R.area = R.border_pixels = R.edges_r = R.edges_c = R.perim_n1 = R.perim_n2 = R.perim_n3 = R.hull_area2 = R.feret_max_d2 = 0;
    R.n_vertices = R.flags = 0;
    *out = R;
}

__device__ __forceinline__ int64_t vertex_slots(int h, int w)
{
    return h < 1 || w < 1 ? 0 : 2 * (int64_t)(h + 1 < 2 * w + 2 ? h + 1 : 2 * w + 2);
}

__global__ __launch_bounds__(STPB) void k_shape_objects(SetLabels S, const int32_t *obj_image, const int32_t *boxes, const int64_t *bits_off,
                                                        const uint32_t *bits_, const int64_t *slot_off, int32_t *slots, sdsm_shape_record *out)
{
    __shared__ ShapeLds T;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int im = obj_image ? obj_image[i] : 0;
    Fragment f;
    if (!fragment_box(S, im, boxes, i, f)) {
        if (tid == 0) zero_record(out + i);      // (uniform: the whole workgroup leaves; no bit of the fragment is read)
        return;
    }
    const int H = f.H, W = f.W, br0 = f.r0, bc0 = f.c0, h = f.h, w = f.w;
    const uint32_t *bits = bits_ + bits_off[i];
    const uint32_t n_words = ((uint32_t)h * (uint32_t)w + 31) >> 5;
    const int WR = (w + 31) >> 5;                // words of a row
    const int TW = WR < TWMAX ? WR : TWMAX;      // words of a column tile
    const int WS = TW + 2;                       // LDS stride of a row: the tile and a halo word on either side
    int B = (PE_WORDS / WS - 6) / 2;             // rows of a band: (B + 4) rows of P and (B + 2) rows of E
    B = B > BMAX ? BMAX : B;
    B = B > h ? h : B;
    uint32_t *P = T.pe, *E = T.pe + (B + 4) * WS;
    if (tid == 0) {
        for (int k = 0; k < 7; k++) T.cnt[k] = 0;
        T.area2 = T.d2max = 0;
        T.overflow = 0;
        T.first[0] = INT_MAX; T.last[0] = -1;
    }
    uint32_t area = 0, border = 0, e_r = 0, e_c = 0, n1 = 0, n2 = 0, n3 = 0;
    int nl = 0, nr = 0, rmin = -1, rmax = -1, cmin = INT_MAX, cmax = -1;     // (thread 0: nl, rows, cmin; thread 64: nr, cmax)
    for (int r0 = 0; r0 < h; r0 += B) {
        const int nb = h - r0 < B ? h - r0 : B;
        for (int k = 1 + tid; k <= nb + 1; k += STPB) { T.first[k] = INT_MAX; T.last[k] = -1; }
        for (int j0 = 0; j0 < WR; j0 += TW) {
            const int tw = WR - j0 < TW ? WR - j0 : TW, tws = tw + 2;
            __syncthreads();                     // the tile before is done with P and E; first / last are set up
            for (int idx = tid; idx < (nb + 4) * tws; idx += STPB) {                 // P: rows r0 - 2 .. r0 + nb + 1, words j0 - 1 .. j0 + tw
                const int pr = idx / tws, jj = idx - pr * tws;
                P[pr * WS + jj] = window_word(bits, n_words, h, w, r0 - 2 + pr, j0 - 1 + jj);
            }
            __syncthreads();
            for (int idx = tid; idx < (nb + 2) * tws; idx += STPB) {                 // E: rows r0 - 1 .. r0 + nb, the same words
                const int er = idx / tws, jj = idx - er * tws, pr = er + 1;
                const uint32_t p = P[pr * WS + jj];
                uint32_t e = 0;
                if (p) {
                    const uint32_t u = P[(pr - 1) * WS + jj], d = P[(pr + 1) * WS + jj];
                    const uint32_t pl = jj > 0 ? P[pr * WS + jj - 1] : 0u, pn = jj < tw + 1 ? P[pr * WS + jj + 1] : 0u;
                    const uint32_t lf = (p << 1) | (pl >> 31), rt = (p >> 1) | (pn << 31);
                    // (a halo word lacks its outer neighbour: its bit next to the tile, the only one used, does not depend on it)
                    e = p & ~(u & d & lf & rt);
                    if (er >= 1 && er <= nb && jj >= 1 && jj <= tw) {                // a word of the band and the tile: counted once
                        area += __popc(p); border += __popc(e);
                        e_r += __popc(p & ~u) + __popc(p & ~d);
                        e_c += __popc(p & ~lf) + __popc(p & ~rt);
                        const int c = 32 * (j0 + jj - 1);
                        atomicMin(&T.first[er], c + __builtin_ctz(p));
                        atomicMax(&T.last[er], c + 31 - __builtin_clz(p));
                    }
                }
                E[er * WS + jj] = e;
            }
            __syncthreads();
            for (int idx = tid; idx < nb * tw; idx += STPB) {                        // classes: the border pixels of the band and the tile
                const int q = idx / tw, er = 1 + q, jj = 1 + idx - q * tw;
                const uint32_t *row = E + er * WS + jj;
                const uint32_t e = row[0];
                if (!e) continue;
                const uint32_t eu = row[-WS], ed = row[WS];
                const uint32_t o_l = (e << 1) | (row[-1] >> 31), o_r = (e >> 1) | (row[1] << 31);
                const uint32_t ul = (eu << 1) | (row[-WS - 1] >> 31), ur = (eu >> 1) | (row[-WS + 1] << 31);
                const uint32_t dl = (ed << 1) | (row[WS - 1] >> 31), dr = (ed >> 1) | (row[WS + 1] << 31);
                uint32_t o0, o1, o2, d0, d1, d2;
                sum4(eu, ed, o_l, o_r, o0, o1, o2);
                sum4(ul, ur, dl, dr, d0, d1, d2);
                const uint32_t o_is0 = ~(o0 | o1 | o2), o_is1 = o0 & ~o1 & ~o2;
                n1 += __popc(e & o1 & ~o2 & ~d2 & ~(d1 & d0));                       // 2 or 3 orthogonal, at most 2 diagonal
                n2 += __popc(e & ~d2 & d1 & ((o_is0 & ~d0) | (o_is1 & d0)));         // (0, 2) and (1, 3)
                n3 += __popc(e & o_is1 & ~d2 & (d0 ^ d1));                           // (1, 1) and (1, 2)
            }
        }
        __syncthreads();                         // the extents of the band's rows are complete
        const bool last_band = r0 + nb == h;
        if (tid == 0) {                          // lattice rows r0 .. r0 + nb - 1 (and h behind the last band): pixel rows y - 1 and y
            for (int y = r0; y < r0 + nb + (last_band ? 1 : 0); y++) {
                const int a = T.first[y - r0], b = T.first[y - r0 + 1];
                if (b != INT_MAX) { if (rmin < 0) rmin = y; rmax = y; cmin = b < cmin ? b : cmin; }
                const int x = a < b ? a : b;
                if (x != INT_MAX) chain_push(T.chain_l, nl, y, x, 1, &T.overflow);
            }
            T.first[0] = T.first[nb];
        } else if (tid == 64) {
            for (int y = r0; y < r0 + nb + (last_band ? 1 : 0); y++) {
                const int a = T.last[y - r0], b = T.last[y - r0 + 1];
                cmax = b > cmax ? b : cmax;
                const int x = a > b ? a : b;
                if (x >= 0) chain_push(T.chain_r, nr, y, x + 1, -1, &T.overflow);
            }
            T.last[0] = T.last[nb];
        }
        __syncthreads();
    }
    // the counts of the workgroup
    uint32_t c7[7] = {area, border, e_r, e_c, n1, n2, n3};
#pragma unroll
    for (int k = 0; k < 7; k++) {
        uint32_t v = c7[k];                      // (a thread sees fewer than 2^23 pixels: a wavefront's sum fits 32 bits)
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((tid & 63) == 0 && v) atomicAdd(&T.cnt[k], (u64)v);
    }
    if (tid == 0) { T.nl = nl; T.rmin = rmin; T.rmax = rmax; T.cmin = cmin; }
    if (tid == 64) { T.nr = nr; T.cmax = cmax; }
    __syncthreads();
    // the hull: left chain downwards, right chain upwards
    nl = T.nl; nr = T.nr;
    const int nv = nl + nr;
    const int64_t cap = vertex_slots(h, w);
    i64 a2 = 0;
    u64 dm = 0;
    int32_t *my = slots + 2 * slot_off[i];
    for (int k = tid; k < nv; k += STPB) {
        const uint32_t p = k < nl ? T.chain_l[k] : T.chain_r[nr - 1 - (k - nl)];
        const int k1 = k + 1 == nv ? 0 : k + 1;
        const uint32_t q = k1 < nl ? T.chain_l[k1] : T.chain_r[nr - 1 - (k1 - nl)];
        const i64 py = p >> 16, px = p & 0xffffu, qy = q >> 16, qx = q & 0xffffu;
        a2 += py * qx - px * qy;
        for (int m = k + 1; m < nv; m++) {
            const uint32_t t = m < nl ? T.chain_l[m] : T.chain_r[nr - 1 - (m - nl)];
            const i64 dy = (i64)(t >> 16) - py, dx = (i64)(t & 0xffffu) - px;
            const u64 d = (u64)(dy * dy + dx * dx);
            dm = d > dm ? d : dm;
        }
        if (k < cap) { my[2 * k] = br0 + (int)py; my[2 * k + 1] = bc0 + (int)px; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        a2 += __shfl_down(a2, o);
        const u64 t = __shfl_down(dm, o);
        dm = t > dm ? t : dm;
    }
    if ((tid & 63) == 0) { atomicAdd(&T.area2, (u64)a2); atomicMax(&T.d2max, dm); }
    __syncthreads();
    if (tid == 0) {
        sdsm_shape_record R;
        R.area = (i64)T.cnt[0]; R.border_pixels = (i64)T.cnt[1]; R.edges_r = (i64)T.cnt[2]; R.edges_c = (i64)T.cnt[3];
        R.perim_n1 = (i64)T.cnt[4]; R.perim_n2 = (i64)T.cnt[5]; R.perim_n3 = (i64)T.cnt[6];
        R.hull_area2 = (i64)T.area2; R.feret_max_d2 = (i64)T.d2max;
        R.n_vertices = nv;
        const bool frame = nv > 0 && (br0 + T.rmin == 0 || bc0 + T.cmin == 0 || br0 + T.rmax + 1 == H || bc0 + T.cmax + 1 == W);
        R.flags = (frame ? 1 : 0) | (T.overflow ? (1 << 30) : 0);
        out[i] = R;
    }
}

// one workgroup: vert_off[k] = n_vertices of the objects before k, vert_off[n] = all.  Thread t sums a run of consecutive objects.
__global__ __launch_bounds__(STPB) void k_shape_offsets(int n, const sdsm_shape_record *recs, int64_t *vert_off)
{
    __shared__ int64_t part[STPB];
    const int tid = threadIdx.x, chunk = (n + STPB - 1) / STPB;
    const int64_t lo = (int64_t)tid * chunk, hi = lo + chunk < n ? lo + chunk : n;
    int64_t s = 0;
    for (int64_t k = lo; k < hi; k++) s += recs[k].n_vertices;
    part[tid] = s;
    __syncthreads();
    int64_t base = 0;
    for (int k = 0; k < tid; k++) base += part[k];
    for (int64_t k = lo; k < hi; k++) { vert_off[k] = base; base += recs[k].n_vertices; }
    if (tid == STPB - 1) vert_off[n] = base;
}

__global__ __launch_bounds__(STPB) void k_shape_gather(const sdsm_shape_record *recs, const int32_t *boxes, const int64_t *slot_off, const int32_t *slots,
                                                       const int64_t *vert_off, int32_t *verts)
{
    const int i = blockIdx.x;
    int64_t nv = recs[i].n_vertices;
    const int64_t cap = vertex_slots(boxes[4 * i + 2], boxes[4 * i + 3]);
    nv = nv > cap ? cap : nv;                    // (never: a chain holds at most min(h + 1, 2 w + 2) vertices)
    const int2 *src = (const int2 *)slots + slot_off[i];
    int2 *dst = (int2 *)verts + vert_off[i];
    for (int64_t k = threadIdx.x; k < nv; k += STPB) dst[k] = src[k];
}

// label form: the bit of every pixel in the window of its label
__global__ __launch_bounds__(STPB) void k_shape_scatter(SetLabels S, const int32_t *labels_, const int32_t *label_obj_, int n, const int32_t *boxes,
                                                        const int64_t *bits_off, int64_t window_words, uint32_t *bits, int32_t *bad)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int W = S.W[im], n_labels = S.n_labels[im];
    const int64_t px = (int64_t)S.H[im] * W;
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * SBAND + (int64_t)threadIdx.x * SSEG;
    if (p0 >= px) return;
    const int32_t *lab = labels_ + S.off[im];
    const int32_t *label_obj = label_obj_ + S.rec_off[im];
    const int cnt = px - p0 < SSEG ? (int)(px - p0) : SSEG;
    int r = (int)(p0 / W), c = (int)(p0 % W);
    int32_t cur_l = -1;                          // the label whose window the registers describe; -1: none
    int b_r0 = 0, b_c0 = 0, b_h = 0, b_w = 0, n_bad = 0;
    int64_t b_off = 0, cur_word = -1;
    uint32_t mask = 0;
    for (int k = 0; k < cnt; k++) {
        const int32_t l = lab[p0 + k];
        if (l != cur_l) {
            cur_l = l;
            b_h = 0;
            if (l >= 0 && l < n_labels) {
                const int obj = label_obj[l];
                if (obj >= 0 && obj < n) { b_r0 = boxes[4 * obj]; b_c0 = boxes[4 * obj + 1]; b_h = boxes[4 * obj + 2]; b_w = boxes[4 * obj + 3]; b_off = bits_off[obj]; }
            }
        }
        if (l < 0 || l >= n_labels) n_bad++;
        const int rr = r - b_r0, cc = c - b_c0;
        if (b_h > 0 && rr >= 0 && rr < b_h && cc >= 0 && cc < b_w) {
            const uint32_t bit = (uint32_t)rr * (uint32_t)b_w + (uint32_t)cc;
            const int64_t word = b_off + (bit >> 5);
            if (word != cur_word) {
                if (mask && cur_word >= 0 && cur_word < window_words) atomicOr(bits + cur_word, mask);
                cur_word = word; mask = 0;
            }
            mask |= 1u << (bit & 31);
        }
        if (++c == W) { c = 0; r++; }
    }
    if (mask && cur_word >= 0 && cur_word < window_words) atomicOr(bits + cur_word, mask);
    if (n_bad) atomicAdd(bad + im, n_bad);
}

}  // namespace

extern "C" int64_t sdsm_shape_vertex_slots(int h, int w)
{
    return h < 1 || w < 1 ? 0 : 2 * (int64_t)(h + 1 < 2 * w + 2 ? h + 1 : 2 * w + 2);
}

extern "C" hipError_t sdsm_shape_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                              const int64_t *bits_off, const uint32_t *bits, const int64_t *slot_off, int32_t *slots,
                                              sdsm_shape_record *out, int64_t *vert_off, int32_t *verts, hipStream_t stream)
{
    const SetLabels S = make_set(images, n_images);
    if (n > 0) hipLaunchKernelGGL(k_shape_objects, dim3(n), dim3(STPB), 0, stream, S, obj_image, boxes, bits_off, bits, slot_off, slots, out);
    hipLaunchKernelGGL(k_shape_offsets, dim3(1), dim3(STPB), 0, stream, n, out, vert_off);
    if (n > 0) hipLaunchKernelGGL(k_shape_gather, dim3(n), dim3(STPB), 0, stream, out, boxes, slot_off, slots, vert_off, verts);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_shape_scatter_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int64_t *rec_off,
                                              const int32_t *n_labels, const int32_t *label_obj, int n, const int32_t *boxes, const int64_t *bits_off,
                                              int64_t window_words, uint32_t *bits, int32_t *bad, hipStream_t stream)
{
    SetLabels S = make_set(images, n_images);
    for (int i = 0; i < n_images; i++) {
        S.rec_off[i] = rec_off[i]; S.n_labels[i] = n_labels[i];
        S.start[i + 1] = S.start[i] + (int32_t)(((int64_t)S.H[i] * S.W[i] + SBAND - 1) / SBAND);
    }
    hipError_t e = hipMemsetAsync(bad, 0, (size_t)n_images * sizeof(int32_t), stream);
    if (e == hipSuccess && window_words > 0) e = hipMemsetAsync(bits, 0, (size_t)window_words * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shape_scatter, dim3(S.start[n_images]), dim3(STPB), 0, stream, S, labels, label_obj, n, boxes, bits_off, window_words, bits, bad);
    return hipGetLastError();
}
