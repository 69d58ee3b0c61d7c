// Label maps and result overlays of a segmentation on the GPU (superdsm/render.py:137-451), for one image or a set of images.
//
// Reference behaviour restated here (never its code); the definition every kernel is tested against is superdsm_amd/render.py:
//   rasterize_objects    render.py:368-385   k_morph: disk dilation / erosion of every object in a window of its box
//   rasterize_labels     render.py:398-405   k_overlaps: |A n B| of the pairs whose windows intersect (integers; the division stays on the host)
//                        render.py:425-431   k_paint_max / k_paint_mark / k_paint_target: highest label per pixel, overlap pixels zeroed
//                        render.py:432-433   k_compact: the overlap pixels and the marker pixels next to one, for the host flood
//                        render.py:443-447   k_lost / k_fill: objects that the flood left without a label
//                        render.py:449       k_finish: uint16 with the background label
//   rasterize_regions, render_regions_over_image, render_result_over_image
//                        render.py:246-365   k_overlay: disk minimum / maximum of the label image through LDS, fused with the painting
//   render_ymap          render.py:123-134   k_colormap (source 0): clip, subtract, divide, colour-map lookup
//   shuffle_labels, colorize_labels
//                        render.py:462-508   k_label_range (minimum / maximum of the permuted labels), k_colormap (source 1), k_permute
//   draw_line, render_adjacencies
//                        render.py:13-99     k_graph_mark (one workgroup per seed or line), k_graph_paint
//
// Objects arrive as sdsm_post_objects takes them: a box (r0, c0, h, w) in the coordinates of their image and the h * w bits of the
// fragment, row-major, LSB first in uint32 words.  Every atomic is an integer atomic (max, add, or) whose result does not depend on
// the arrival order, so every launch gives the same bytes.
//
// Image sets: the objects of all images form one list (d_obj_image names the image of each), the pixel buffers are packed as the
// sdsm_set_image table says; one launch per phase serves the whole set and runs the __device__ bodies of the single-image case, which
// is a set of one image.
#include "sdsm_common.h"
#include "sdsm_set.h"
#include <climits>

#pragma clang fp contract(off)   // the blend of the discarded regions is numpy's a + b * c, unfused

namespace {

constexpr int RTPB = 256;
constexpr int TILE = 32;                         // overlay: TILE x TILE pixels per workgroup, 4 per thread
constexpr int RMAX = 16;                         // largest disk radius (as the mask refinement of sdsm_post_objects)
constexpr int PITCH_MAX = TILE + 2 * RMAX;

struct RSet {                                    // the images of a launch
    int32_t n;
    int32_t H[SDSM_MAX_SET_IMAGES], W[SDSM_MAX_SET_IMAGES];
    int64_t off[SDSM_MAX_SET_IMAGES];            // first pixel of the image in the packed buffers
    int64_t cap_off[SDSM_MAX_SET_IMAGES + 1];    // k_compact: first entry of the image, capacity = the difference
    int32_t start[SDSM_MAX_SET_IMAGES + 1];      // flattened grid: first workgroup of the image
};

struct RObjects {                                // the objects of a launch
    const int32_t *image;                        // image of each object (null: image 0)
    const int32_t *boxes;                        // n x 4: r0, c0, h, w
    const int64_t *bits_off;
    const uint32_t *bits;
};

struct Entry { int32_t idx, label; double dist; };   // sdsm_render_entry

__device__ __forceinline__ bool rbit(const uint32_t *bits, int h, int w, int r, int c)
{
    if (r < 0 || c < 0 || r >= h || c >= w) return false;
    const int b = r * w + c;
    return (bits[b >> 5] >> (b & 31)) & 1u;
}

// sum of an int over the workgroup (LDS integer atomic: order-independent)
__device__ __forceinline__ int block_count(int v, int *sh)
{
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(sh, v);
    __syncthreads();
    const int t = *sh;
    __syncthreads();
    return t;
}

// ---- phase 1: dilation / erosion by disk(|radius|) (render.py:380-384, _morph.py) ------------------------------------------------
__global__ __launch_bounds__(RTPB) void k_morph(RSet S, RObjects O, int radius, const int64_t *new_off, uint32_t *new_bits, int32_t *area)
{
    __shared__ int sh;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int im = O.image ? O.image[i] : 0;
    const int H = S.H[im], W = S.W[im];
    const int r0 = O.boxes[4 * i], c0 = O.boxes[4 * i + 1], h = O.boxes[4 * i + 2], w = O.boxes[4 * i + 3];
    const uint32_t *bits = O.bits + O.bits_off[i];
    const int m = radius < 0 ? -radius : radius;
    const int nr0 = r0 - m < 0 ? 0 : r0 - m, nc0 = c0 - m < 0 ? 0 : c0 - m;
    const int nr1 = r0 + h + m > H ? H : r0 + h + m, nc1 = c0 + w + m > W ? W : c0 + w + m;
    const int nw = nc1 - nc0, nh = nr1 - nr0;
    uint32_t *nbits = new_bits + new_off[i];
    for (int e = tid; e < (nh * nw + 31) / 32; e += RTPB) nbits[e] = 0;
    __syncthreads();
    int cnt = 0;
    for (int e = tid; e < nh * nw; e += RTPB) {
        const int r = nr0 + e / nw, c = nc0 + e % nw;
        bool any = false, all = true;
        for (int dr = -m; dr <= m; dr++) for (int dc = -m; dc <= m; dc++) {
            if (dr * dr + dc * dc > m * m) continue;
            const int rr = r + dr, cc = c + dc;
            const bool inside = rr >= 0 && cc >= 0 && rr < H && cc < W;
            const bool b = inside && rbit(bits, h, w, rr - r0, cc - c0);
            any |= b;
            all &= inside ? b : true;            // erosion: outside the image counts as foreground
        }
        if (radius > 0 ? any : all) { atomicOr(&nbits[e >> 5], 1u << (e & 31)); cnt++; }
    }
    const int total = block_count(cnt, &sh);
    if (tid == 0) area[i] = total;
}

// ---- phase 2: |A n B| of a pair of objects of one image (render.py:401) ---------------------------------------------------------
__global__ __launch_bounds__(RTPB) void k_overlaps(RObjects O, const int32_t *pairs, int32_t *inter)
{
    __shared__ int sh;
    const int k = blockIdx.x;
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    const int32_t *A = O.boxes + 4 * a, *B = O.boxes + 4 * b;
    const uint32_t *ba = O.bits + O.bits_off[a], *bb = O.bits + O.bits_off[b];
    const int r0 = A[0] > B[0] ? A[0] : B[0], c0 = A[1] > B[1] ? A[1] : B[1];
    const int r1 = A[0] + A[2] < B[0] + B[2] ? A[0] + A[2] : B[0] + B[2], c1 = A[1] + A[3] < B[1] + B[3] ? A[1] + A[3] : B[1] + B[3];
    const int nh = r1 - r0, nw = c1 - c0;
    int cnt = 0;
    if (nh > 0 && nw > 0)
        for (int e = threadIdx.x; e < nh * nw; e += RTPB) {
            const int r = r0 + e / nw, c = c0 + e % nw;
            cnt += rbit(ba, A[2], A[3], r - A[0], c - A[1]) && rbit(bb, B[2], B[3], r - B[0], c - B[1]);
        }
    const int total = block_count(cnt, &sh);
    if (threadIdx.x == 0) inter[k] = total;
}

// ---- phase 3: paint (render.py:425-431) ----------------------------------------------------------------------------------------
// mode 0: label[p] = max of the labels covering p, cover[p] = 1.  mode 1: cover[p] = 2 where an object with another label covers p
// (the merged objects of one label count once).  mode 2: overlap pixels lose their label; target = result != 0.
// mode 3 (render.py:443-447): lost[label of the object] += its pixels with label 0; vmax[image] = highest label of the image.
// mode 4: the pixels of the objects sel[0 .. n) that have label 0 get new_label; filled += their number.
struct PaintArgs {
    int32_t mode, new_label;
    const int32_t *obj_label;
    const int32_t *sel;
    int32_t *label;
    uint8_t *cover, *target;
    int32_t *lost, *vmax, *filled;
};

__global__ __launch_bounds__(RTPB) void k_paint(RSet S, RObjects O, PaintArgs A)
{
    __shared__ int sh;
    const int i = A.mode == 4 ? A.sel[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int im = O.image ? O.image[i] : 0;
    const int W = S.W[im];
    const int r0 = O.boxes[4 * i], c0 = O.boxes[4 * i + 1], h = O.boxes[4 * i + 2], w = O.boxes[4 * i + 3];
    const uint32_t *bits = O.bits + O.bits_off[i];
    const int l = A.obj_label[i];
    int32_t *label = A.label + S.off[im];
    uint8_t *cover = A.cover ? A.cover + S.off[im] : nullptr, *target = A.target ? A.target + S.off[im] : nullptr;
    int cnt = 0, mx = 0;
    for (int e = tid; e < h * w; e += RTPB) {
        if (!((bits[e >> 5] >> (e & 31)) & 1u)) continue;
        const int r = e / w, c = e - r * w;
        const int64_t p = (int64_t)(r0 + r) * W + (c0 + c);
        switch (A.mode) {
        case 0: atomicMax(&label[p], l); cover[p] = 1; break;
        case 1: if (label[p] != l) cover[p] = 2; break;
        case 2: if (cover[p] == 2) { label[p] = 0; target[p] = 0; } else target[p] = 1; break;
        case 3: { const int v = label[p]; cnt += v == 0; mx = v > mx ? v : mx; } break;
        default: if (label[p] == 0) { label[p] = A.new_label; cnt++; } break;
        }
    }
    if (A.mode < 3) return;
    const int total = block_count(cnt, &sh);
    if (A.mode == 3) {
        if (tid == 0 && total) atomicAdd(&A.lost[l], total);
        if (mx) atomicMax(&A.vmax[im], mx);
    } else if (tid == 0 && total) atomicAdd(A.filled, total);
}

// ---- phase 5: the sparse set of the flood (render._watershed) --------------------------------------------------------------------
__global__ __launch_bounds__(RTPB) void k_compact(RSet S, const int32_t *label_, const uint8_t *cover_, const double *dist_, Entry *entries, int32_t *counts)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int H = S.H[im], W = S.W[im];
    const int64_t n = (int64_t)H * W, p = (int64_t)(blockIdx.x - S.start[im]) * RTPB + threadIdx.x;
    if (p >= n) return;
    const uint8_t *cover = cover_ + S.off[im];
    const uint8_t cv = cover[p];
    if (cv == 0) return;
    const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
    bool take = cv == 2;
    if (!take)                                    // a marker pixel with an overlap pixel among its 4-neighbours
        take = (r > 0 && cover[p - W] == 2) || (r + 1 < H && cover[p + W] == 2) || (c > 0 && cover[p - 1] == 2) || (c + 1 < W && cover[p + 1] == 2);
    if (!take) return;
    const int64_t cap = S.cap_off[im + 1] - S.cap_off[im];
    const int k = atomicAdd(&counts[im], 1);
    if (k < cap) {
        Entry en;
        en.idx = (int32_t)p; en.label = cv == 2 ? 0 : label_[S.off[im] + p]; en.dist = dist_[S.off[im] + p];
        entries[S.cap_off[im] + k] = en;
    }
}

__global__ void k_scatter(int64_t n, const int64_t *pix, const int32_t *lab, int32_t *label)
{
    const int64_t t = (int64_t)blockIdx.x * RTPB + threadIdx.x;
    if (t < n) label[pix[t]] = lab[t];
}

// ---- phase 7: uint16 with the background label (render.py:449) --------------------------------------------------------------------
__global__ void k_finish(int64_t n, const int32_t *label, uint16_t bg, uint16_t *out)
{
    const int64_t t = (int64_t)blockIdx.x * RTPB + threadIdx.x;
    if (t < n) { const int32_t v = label[t]; out[t] = v == 0 ? bg : (uint16_t)v; }
}

// ---- overlays (render.py:246-365) ---------------------------------------------------------------------------------------------
// mn / mx: minimum / maximum label over the in-image pixels of disk(radius) around a pixel.  Pixels outside the image are loaded
// clamped to the edge: the clamped pixel lies in the image and, being nearer to the centre in both coordinates, in the disk, so it
// changes neither mn nor mx.
//   kind 0 (rasterize_regions + render_regions_over_image): mn != mx -> color; mn == mx == background_label -> blended with bg;
//           uint8 by truncation.
//   kind 1 (render_result_over_image, 'center'): mx > 0 and mn != mx -> color; uint8 by rounding to even.
//   kind 2 ('inner'): label > 0 and mn != mx.
//   kind 3 (rasterize_regions alone): one byte per pixel, bit 0 = border (mn != mx), bit 1 = background (mn == mx == background_label).
struct OverlayArgs {
    int32_t kind, radius, channels, has_bg, background_label;
    int8_t half[2 * RMAX + 1];                  // half width of the disk's row dr at half[dr + radius] (host: make_half)
    double color[3], bg_add[3], bg_keep;        // bg_add = bg[i] * bg[3], bg_keep = 1 - bg[3]
    const int32_t *labels;
    const double *base;                         // channels (1 or 3) float64 per pixel
    uint8_t *out;                               // 3 uint8 per pixel (kind 3: 1)
};

__global__ __launch_bounds__(RTPB) void k_overlay(RSet S, OverlayArgs A)
{
    __shared__ int32_t tile[PITCH_MAX * PITCH_MAX];
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int H = S.H[im], W = S.W[im];
    const int tiles_x = (W + TILE - 1) / TILE;
    const int t = blockIdx.x - S.start[im];
    const int tr0 = (t / tiles_x) * TILE, tc0 = (t % tiles_x) * TILE;
    const int R = A.radius, pitch = TILE + 2 * R;
    const int32_t *labels = A.labels + S.off[im];
    for (int e = threadIdx.x; e < pitch * pitch; e += RTPB) {
        int r = tr0 - R + e / pitch, c = tc0 - R + e % pitch;
        r = r < 0 ? 0 : (r >= H ? H - 1 : r);
        c = c < 0 ? 0 : (c >= W ? W - 1 : c);
        tile[e] = labels[(int64_t)r * W + c];
    }
    __syncthreads();
    const int lx = threadIdx.x & (TILE - 1), ly0 = threadIdx.x >> 5;       // 8 rows of 32 threads, 4 passes
    for (int ly = ly0; ly < TILE; ly += RTPB / TILE) {
        const int r = tr0 + ly, c = tc0 + lx;
        if (r >= H || c >= W) continue;
        const int32_t *ctr = tile + (ly + R) * pitch + (lx + R);
        int32_t mn = *ctr, mx = *ctr;
        for (int dr = -R; dr <= R; dr++) {
            const int s = A.half[dr + R];
            const int32_t *row = ctr + dr * pitch;
            for (int dc = -s; dc <= s; dc++) { const int32_t v = row[dc]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
        }
        const bool diff = mn != mx;
        const bool border = (A.kind == 0 || A.kind == 3) ? diff : (A.kind == 1 ? (mx > 0 && diff) : (*ctr > 0 && diff));
        const bool back = (A.kind == 0 || A.kind == 3) && A.has_bg && !diff && mn == A.background_label;
        const int64_t p = (int64_t)r * W + c;
        if (A.kind == 3) { A.out[S.off[im] + p] = (uint8_t)((border ? 1 : 0) | (back ? 2 : 0)); continue; }
        const double *b = A.base + (S.off[im] + p) * A.channels;
        uint8_t *o = A.out + (S.off[im] + p) * 3;
        for (int ch = 0; ch < 3; ch++) {
            double v = b[A.channels == 3 ? ch : 0];
            if (border) v = A.color[ch];
            else if (back) v = A.bg_add[ch] + v * A.bg_keep;
            v = 255 * v;
            if (A.kind != 0) v = rint(v);
            v = v < 0 ? 0 : (v > 255 ? 255 : v);                           // (NaN passes through both tests; numpy's cast of NaN is undefined)
            o[ch] = (uint8_t)v;
        }
    }
}

// ---- colour maps (render.py:102-134 render_ymap, :454-508 shuffle_labels / colorize_labels) ---------------------------------------
// The lookup is matplotlib's Colormap.__call__ for float input (colors.py, _get_rgba_and_mask): xa = x * N; xa == N -> N - 1;
// xa < 0 -> under (entry N); xa >= N -> over (N + 1); NaN -> bad (N + 2); otherwise the entry (int)xa, truncated.  -0.0 is not < 0
// and reads entry 0; -inf / +inf are under / over.
struct CmapArgs {
    int32_t source;                              // 0: float64 values, 1: int32 labels
    int32_t N;                                   // entries of the colour map; the table has N + 3 rows of 4 float64
    int32_t has_bg, bg_label;
    double bg_color[3];
    double sub[SDSM_MAX_SET_IMAGES], div[SDSM_MAX_SET_IMAGES];   // source 0, per image: x = (clip(y, lo, hi) - sub) / div
    double lo[SDSM_MAX_SET_IMAGES], hi[SDSM_MAX_SET_IMAGES];
    int64_t perm_off[SDSM_MAX_SET_IMAGES + 1];   // source 1, per image: its permutation table is perm[perm_off[i] .. perm_off[i + 1])
    int32_t perm_min[SDSM_MAX_SET_IMAGES];       //   indexed by label - perm_min[i]; a label outside the table reads 0 (render.py:469)
    const double *lut;
    const void *src;
    const int32_t *perm;                         // null: the labels as they are
    const int32_t *range;                        // source 1: minimum, maximum per image (k_label_range)
    int32_t *flags;                              // source 0: bit 0 set per image that holds a NaN
    double *out;                                 // 3 float64 per pixel
};

constexpr int CMAP_PIX = 2048;                   // pixels per workgroup: the table is loaded into LDS once for them

__device__ __forceinline__ int32_t permuted(const int32_t *perm, int64_t off, int64_t n, int32_t lo, int32_t l)
{
    if (!perm) return l;
    const int64_t k = (int64_t)l - lo;
    return (k >= 0 && k < n) ? perm[off + k] : 0;
}

__global__ __launch_bounds__(RTPB) void k_label_range_init(int n, int32_t *range)
{
    const int i = blockIdx.x * RTPB + threadIdx.x;
    if (i < n) { range[2 * i] = INT_MAX; range[2 * i + 1] = INT_MIN; }
}

__global__ __launch_bounds__(RTPB) void k_label_range(RSet S, CmapArgs A, int32_t *range)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int64_t px = (int64_t)S.H[im] * S.W[im];
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * CMAP_PIX;
    const int32_t *lab = (const int32_t *)A.src + S.off[im];
    const int64_t pn = A.perm_off[im + 1] - A.perm_off[im];
    int32_t mn = INT_MAX, mx = INT_MIN;
    for (int e = threadIdx.x; e < CMAP_PIX; e += RTPB) {
        const int64_t p = p0 + e;
        if (p >= px) break;
        const int32_t l = permuted(A.perm, A.perm_off[im], pn, A.perm_min[im], lab[p]);
        mn = l < mn ? l : mn; mx = l > mx ? l : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t a = __shfl_down(mn, o), b = __shfl_down(mx, o);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0 && mn <= mx) { atomicMin(range + 2 * im, mn); atomicMax(range + 2 * im + 1, mx); }
}

// shuffle_labels alone: out[p] = the permuted label
__global__ __launch_bounds__(RTPB) void k_permute(RSet S, CmapArgs A, int32_t *out)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int64_t px = (int64_t)S.H[im] * S.W[im];
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * CMAP_PIX;
    const int32_t *lab = (const int32_t *)A.src + S.off[im];
    const int64_t pn = A.perm_off[im + 1] - A.perm_off[im];
    for (int e = threadIdx.x; e < CMAP_PIX; e += RTPB) {
        const int64_t p = p0 + e;
        if (p >= px) break;
        out[S.off[im] + p] = permuted(A.perm, A.perm_off[im], pn, A.perm_min[im], lab[p]);
    }
}

// One thread per OUTPUT element (pixel, channel): consecutive lanes store consecutive float64, the three lanes of a pixel read the
// same source element.  The table (3 of its 4 columns) sits in LDS.
__global__ __launch_bounds__(RTPB) void k_colormap(RSet S, CmapArgs A)
{
    extern __shared__ double lut[];              // (N + 3) x 3
    const int N = A.N;
    for (int e = threadIdx.x; e < (N + 3) * 3; e += RTPB) lut[e] = A.lut[(e / 3) * 4 + e % 3];
    __syncthreads();
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int64_t px = (int64_t)S.H[im] * S.W[im];
    const int64_t p0 = (int64_t)(blockIdx.x - S.start[im]) * CMAP_PIX;
    double *out = A.out + 3 * S.off[im];
    const double lo = A.lo[im], hi = A.hi[im], sub = A.sub[im], div = A.div[im];
    int32_t mn = 0, mx = 0;
    const int64_t pn = A.perm_off[im + 1] - A.perm_off[im];
    if (A.source == 1) { mn = A.range[2 * im]; mx = A.range[2 * im + 1]; }
    const double span = (double)((int64_t)mx - mn);
    bool nan_seen = false;
    for (int e = threadIdx.x; e < 3 * CMAP_PIX; e += RTPB) {
        const int64_t p = p0 + e / 3;
        if (p >= px) break;
        const int ch = e % 3;
        double x;
        bool back = false;
        if (A.source == 0) {
            double v = ((const double *)A.src)[S.off[im] + p];
            nan_seen |= v != v;
            v = v < lo ? lo : v;                 // numpy's clip: minimum(maximum(v, lo), hi), a NaN stays
            v = v > hi ? hi : v;
            x = (v - sub) / div;
        } else {
            const int32_t l = permuted(A.perm, A.perm_off[im], pn, A.perm_min[im], ((const int32_t *)A.src)[S.off[im] + p]);
            back = A.has_bg && l == A.bg_label;
            x = (double)((int64_t)l - mn) / span;    // 0 / 0 = NaN where the image holds one label: the "bad" colour
        }
        double xa = x * N;
        if (xa == (double)N) xa = N - 1;
        int idx;
        if (xa != xa) idx = N + 2;
        else if (xa < 0) idx = N;
        else if (xa >= (double)N) idx = N + 1;
        else idx = (int)xa;
        out[3 * p + ch] = back ? A.bg_color[ch] : lut[3 * idx + ch];
    }
    if (nan_seen) atomicOr(A.flags + im, 1);
}

// ---- adjacency graphs (render.py:13-99 draw_line, render_adjacencies) ------------------------------------------------------------
// Painting order of the definition: every rim, then the lines in list order, then every disk.  Pass 1 takes, per pixel, the integer
// maximum of a key that grows in that order (KEY_RIM < line keys growing with the line's index < KEY_DISK); pass 2 paints from the
// key.  The maximum does not depend on the arrival order.  A line's key carries in bit 0 whether the pixel lies in the line's core
// (value 1) or in the ring of a fractional thickness (render.py:40-44: one value for the whole ring, computed on the host), so
// pass 2 recomputes nothing: a line reaches a pixel once, through one candidate of its band.
//
// Line pixels (what skimage.draw.line documents): the longer axis drives (columns on a tie), one pixel per step i = 0 .. dl; the error
// term starts at 2 ds - dl, gains 2 ds per step and, while >= 0 after a pixel, the minor coordinate steps and the term loses 2 dl.
// As ds <= dl, the minor offset before pixel i is the smallest m with 2 ds i - dl - 2 dl m < 0: m_i = floor((2 ds i + dl) / (2 dl)),
// which also gives m_dl = ds, the end point.  (dl = 0: the single pixel.)
//
// Thick line: pixels whose squared distance to the nearest line pixel is <= d2 (an integer the host derives from the definition's
// sqrt(d2) < threshold).  With n = reach = floor(sqrt(d2)), the nearest line pixel of a pixel at driving coordinate k lies at a
// step j with |j - k| <= n, and |m_j - m_clamp(k)| <= |j - clamp(k)| <= n, so the band minor = m_clamp(k) + [-2 n, 2 n] holds every
// pixel the line can reach.  The m_j of a chunk of steps sit in LDS.
constexpr int32_t KEY_RIM = 1, KEY_LINE = 1 << 20, KEY_DISK = 1 << 21;
constexpr int GRAPH_REACH_MAX = 16;              // line thickness <= 33
constexpr int GRAPH_CHUNK = 1024;                // driving steps per LDS chunk

struct GraphArgs {
    int32_t n_prims, seed_reach, line_reach, core_d2, ring_d2, channels;
    double rim_radius, disk_radius;
    double colors[12];                           // rim, disk, line core, line ring
    const int32_t *prims;                        // 8 int32 each: kind (0 seed, 1 line), index, image, r0, c0, r1, c1, 0
    const double *base;
    int32_t *key;
    uint8_t *out;
};

__global__ __launch_bounds__(RTPB) void k_graph_mark(RSet S, GraphArgs A)
{
    __shared__ int32_t minor[GRAPH_CHUNK + 2 * GRAPH_REACH_MAX];
    const int32_t *P = A.prims + 8 * (int64_t)blockIdx.x;
    const int kind = P[0], index = P[1] & 0xFFFF, im = P[2];
    if (im < 0 || im >= S.n) return;
    const int H = S.H[im], W = S.W[im];
    int32_t *key = A.key + S.off[im];
    const int r0 = P[3], c0 = P[4], r1 = P[5], c1 = P[6];
    if (kind == 0) {                             // a seed: rim and disk, ((r - r0) / radius)^2 + ((c - c0) / radius)^2 < 1, as written
        const int R = A.seed_reach, side = 2 * R + 1;
        for (int e = threadIdx.x; e < side * side; e += RTPB) {
            const int r = r0 - R + e / side, c = c0 - R + e % side;
            if (r < 0 || c < 0 || r >= H || c >= W) continue;
            const double dr = (double)(r - r0), dc = (double)(c - c0);
            const double ar = dr / A.disk_radius, ac = dc / A.disk_radius, br = dr / A.rim_radius, bc = dc / A.rim_radius;
            const bool in_disk = ar * ar + ac * ac < 1.0, in_rim = br * br + bc * bc < 1.0;
            if (in_disk) atomicMax(key + (int64_t)r * W + c, KEY_DISK);
            else if (in_rim) atomicMax(key + (int64_t)r * W + c, KEY_RIM);
        }
        return;
    }
    const int adr = r1 > r0 ? r1 - r0 : r0 - r1, adc = c1 > c0 ? c1 - c0 : c0 - c1;
    const bool steep = adr > adc;
    const int dl = steep ? adr : adc, ds = steep ? adc : adr;
    const int sr = r1 - r0 > 0 ? 1 : -1, sc = c1 - c0 > 0 ? 1 : -1;
    const int sl = steep ? sr : sc, ss = steep ? sc : sr;
    const int l0 = steep ? r0 : c0, s0 = steep ? c0 : r0;
    const int n = A.line_reach, width = 4 * n + 1;
    for (int a = -n; a <= dl + n; a += GRAPH_CHUNK) {          // candidates with driving step k in [a, a + CHUNK)
        const int j0 = a - n < 0 ? 0 : a - n;                  // the steps whose pixels they can reach: j0 .. j1
        const int j1 = a + GRAPH_CHUNK - 1 + n > dl ? dl : a + GRAPH_CHUNK - 1 + n;
        __syncthreads();
        for (int j = j0 + threadIdx.x; j <= j1; j += RTPB)
            minor[j - j0] = dl == 0 ? 0 : (int32_t)((2 * (int64_t)ds * j + dl) / (2 * (int64_t)dl));
        __syncthreads();
        const int k_end = a + GRAPH_CHUNK - 1 > dl + n ? dl + n : a + GRAPH_CHUNK - 1;
        const int total = (k_end - a + 1) * width;
        for (int e = threadIdx.x; e < total; e += RTPB) {
            const int k = a + e / width;
            const int kc = k < 0 ? 0 : (k > dl ? dl : k);
            const int m = minor[kc - j0] + e % width - 2 * n;
            const int lc = l0 + sl * k, mc = s0 + ss * m;
            const int r = steep ? lc : mc, c = steep ? mc : lc;
            if (r < 0 || c < 0 || r >= H || c >= W) continue;
            const int ja = k - n < 0 ? 0 : k - n, jb = k + n > dl ? dl : k + n;
            int best = INT_MAX;
            for (int j = ja; j <= jb; j++) {
                const int dj = j - k, dm = minor[j - j0] - m, d2 = dj * dj + dm * dm;
                best = d2 < best ? d2 : best;
            }
            if (best <= A.ring_d2) atomicMax(key + (int64_t)r * W + c, KEY_LINE | (index << 1) | (best <= A.core_d2 ? 1 : 0));
        }
    }
}

__global__ __launch_bounds__(RTPB) void k_graph_paint(RSet S, GraphArgs A)
{
    const int im = set_find(S.start, S.n, blockIdx.x);
    const int64_t px = (int64_t)S.H[im] * S.W[im];
    const int64_t p = (int64_t)(blockIdx.x - S.start[im]) * RTPB + threadIdx.x;
    if (p >= px) return;
    const int32_t k = A.key[S.off[im] + p];
    const double *b = A.base + (S.off[im] + p) * A.channels;
    uint8_t *o = A.out + (S.off[im] + p) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {             // (selects on constant indices: the colours stay in scalar registers)
        double v = b[A.channels == 3 ? ch : 0];
        if (k >= KEY_DISK) v = A.colors[3 + ch];
        else if (k >= KEY_LINE) v = (k & 1) ? A.colors[6 + ch] : A.colors[9 + ch];
        else if (k >= KEY_RIM) v = A.colors[ch];
        v = 255 * v;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);                               // render.py:99, truncation
        o[ch] = (uint8_t)v;
    }
}

RSet make_set(const sdsm_set_image *images, int n_images, int per_block /* pixels per workgroup, 0: none; -1: tiles */)
{
    RSet S{};
    S.n = n_images;
    for (int i = 0; i < n_images; i++) {
        S.H[i] = images[i].H; S.W[i] = images[i].W; S.off[i] = images[i].offset;
        const int64_t px = (int64_t)images[i].H * images[i].W;
        int64_t blocks = 0;
        if (per_block > 0) blocks = (px + per_block - 1) / per_block;
        else if (per_block < 0) blocks = (int64_t)((images[i].H + TILE - 1) / TILE) * ((images[i].W + TILE - 1) / TILE);
        S.start[i + 1] = S.start[i] + (int32_t)blocks;
    }
    return S;
}

RObjects make_objects(const int32_t *image, const int32_t *boxes, const int64_t *bits_off, const uint32_t *bits)
{
    RObjects O{};
    O.image = image; O.boxes = boxes; O.bits_off = bits_off; O.bits = bits;
    return O;
}

}  // namespace

extern "C" hipError_t sdsm_render_morph_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                             const int64_t *bits_off, const uint32_t *bits, int radius, const int64_t *new_off, uint32_t *new_bits,
                                             int32_t *area, hipStream_t stream)
{
    hipLaunchKernelGGL(k_morph, dim3(n), dim3(RTPB), 0, stream, make_set(images, n_images, 0), make_objects(obj_image, boxes, bits_off, bits),
                       radius, new_off, new_bits, area);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_overlaps_impl(int n_pairs, const int32_t *pairs, const int32_t *boxes, const int64_t *bits_off, const uint32_t *bits,
                                                int32_t *inter, hipStream_t stream)
{
    hipLaunchKernelGGL(k_overlaps, dim3(n_pairs), dim3(RTPB), 0, stream, make_objects(nullptr, boxes, bits_off, bits), pairs, inter);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_paint_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                             const int64_t *bits_off, const uint32_t *bits, const int32_t *obj_label, int32_t *label, uint8_t *cover,
                                             uint8_t *target, hipStream_t stream)
{
    const RSet S = make_set(images, n_images, 0);
    const RObjects O = make_objects(obj_image, boxes, bits_off, bits);
    for (int i = 0; i < n_images; i++) {
        const size_t px = (size_t)images[i].H * images[i].W;
        hipError_t e = hipMemsetAsync(label + images[i].offset, 0, px * sizeof(int32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(cover + images[i].offset, 0, px, stream);
        if (e == hipSuccess) e = hipMemsetAsync(target + images[i].offset, 0, px, stream);
        if (e != hipSuccess) return e;
    }
    if (n <= 0) return hipSuccess;
    for (int mode = 0; mode < 3; mode++) {
        PaintArgs A{};
        A.mode = mode; A.obj_label = obj_label; A.label = label; A.cover = cover; A.target = target;
        hipLaunchKernelGGL(k_paint, dim3(n), dim3(RTPB), 0, stream, S, O, A);
    }
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_lost_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                            const int64_t *bits_off, const uint32_t *bits, const int32_t *obj_label, int32_t *label, int32_t *lost,
                                            int n_labels, int32_t *vmax, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(lost, 0, (size_t)(n_labels + 1) * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(vmax, 0, (size_t)n_images * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    PaintArgs A{};
    A.mode = 3; A.obj_label = obj_label; A.label = label; A.lost = lost; A.vmax = vmax;
    hipLaunchKernelGGL(k_paint, dim3(n), dim3(RTPB), 0, stream, make_set(images, n_images, 0), make_objects(obj_image, boxes, bits_off, bits), A);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_fill_impl(const sdsm_set_image *images, int n_images, int n_sel, const int32_t *sel, const int32_t *obj_image,
                                            const int32_t *boxes, const int64_t *bits_off, const uint32_t *bits, const int32_t *obj_label,
                                            int32_t new_label, int32_t *label, int32_t *filled, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(filled, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    PaintArgs A{};
    A.mode = 4; A.new_label = new_label; A.obj_label = obj_label; A.sel = sel; A.label = label; A.filled = filled;
    hipLaunchKernelGGL(k_paint, dim3(n_sel), dim3(RTPB), 0, stream, make_set(images, n_images, 0), make_objects(obj_image, boxes, bits_off, bits), A);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_compact_impl(const sdsm_set_image *images, int n_images, const int32_t *label, const uint8_t *cover, const double *dist,
                                               const int64_t *capacity, void *entries, int32_t *counts, hipStream_t stream)
{
    RSet S = make_set(images, n_images, RTPB);
    for (int i = 0; i < n_images; i++) S.cap_off[i + 1] = S.cap_off[i] + capacity[i];
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_images * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compact, dim3(S.start[n_images]), dim3(RTPB), 0, stream, S, label, cover, dist, (Entry *)entries, counts);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_scatter_impl(int64_t n, const int64_t *pix, const int32_t *lab, int32_t *label, hipStream_t stream)
{
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)((n + RTPB - 1) / RTPB)), dim3(RTPB), 0, stream, n, pix, lab, label);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_finish_impl(int64_t n, const int32_t *label, uint16_t bg, uint16_t *out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_finish, dim3((unsigned)((n + RTPB - 1) / RTPB)), dim3(RTPB), 0, stream, n, label, bg, out);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_overlay_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const double *base, int channels,
                                               int kind, int radius, const double *color, const double *bg, int has_bg, int background_label,
                                               uint8_t *out, hipStream_t stream)
{
    const RSet S = make_set(images, n_images, -1);
    OverlayArgs A{};
    A.kind = kind; A.radius = radius; A.channels = channels; A.has_bg = has_bg; A.background_label = background_label;
    for (int k = 0; k < 3; k++) { A.color[k] = color[k]; A.bg_add[k] = bg ? bg[k] * bg[3] : 0.0; }
    A.bg_keep = bg ? 1 - bg[3] : 1.0;
    for (int dr = -radius; dr <= radius; dr++) {
        int s = 0;
        while ((s + 1) * (s + 1) + dr * dr <= radius * radius) s++;
        A.half[dr + radius] = (int8_t)s;
    }
    A.labels = labels; A.base = base; A.out = out;
    hipLaunchKernelGGL(k_overlay, dim3(S.start[n_images]), dim3(RTPB), 0, stream, S, A);
    return hipGetLastError();
}

static void cmap_tables(CmapArgs &A, int n_images, const int64_t *perm_off, const int32_t *perm_min)
{
    for (int i = 0; i < n_images; i++) {
        A.perm_off[i] = perm_off ? perm_off[i] : 0; A.perm_min[i] = perm_min ? perm_min[i] : 0;
    }
    A.perm_off[n_images] = perm_off ? perm_off[n_images] : 0;
}

extern "C" hipError_t sdsm_render_label_range_impl(const sdsm_set_image *images, int n_images, const int32_t *labels, const int32_t *perm,
                                                   const int64_t *perm_off, const int32_t *perm_min, int32_t *range, int32_t *permuted_out,
                                                   hipStream_t stream)
{
    const RSet S = make_set(images, n_images, CMAP_PIX);
    CmapArgs A{};
    A.source = 1; A.src = labels; A.perm = perm;
    cmap_tables(A, n_images, perm_off, perm_min);
    if (range) {
        hipLaunchKernelGGL(k_label_range_init, dim3(1), dim3(RTPB), 0, stream, n_images, range);
        hipLaunchKernelGGL(k_label_range, dim3(S.start[n_images]), dim3(RTPB), 0, stream, S, A, range);
    }
    if (permuted_out) hipLaunchKernelGGL(k_permute, dim3(S.start[n_images]), dim3(RTPB), 0, stream, S, A, permuted_out);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_colormap_impl(const sdsm_set_image *images, int n_images, int source, const void *src, const double *lut, int N,
                                                const double *clim, const int32_t *perm, const int64_t *perm_off, const int32_t *perm_min,
                                                const int32_t *range, int has_bg, int bg_label, const double *bg_color, int32_t *flags,
                                                double *out, hipStream_t stream)
{
    const RSet S = make_set(images, n_images, CMAP_PIX);
    CmapArgs A{};
    A.source = source; A.N = N; A.has_bg = has_bg; A.bg_label = bg_label;
    for (int k = 0; k < 3; k++) A.bg_color[k] = bg_color ? bg_color[k] : 0.0;
    for (int i = 0; i < n_images && clim; i++) { A.lo[i] = clim[4 * i]; A.hi[i] = clim[4 * i + 1]; A.sub[i] = clim[4 * i + 2]; A.div[i] = clim[4 * i + 3]; }
    cmap_tables(A, n_images, perm_off, perm_min);
    A.lut = lut; A.src = src; A.perm = perm; A.range = range; A.flags = flags; A.out = out;
    if (source == 0) {
        hipError_t e = hipMemsetAsync(flags, 0, (size_t)n_images * sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_colormap, dim3(S.start[n_images]), dim3(RTPB), (size_t)(N + 3) * 3 * sizeof(double), stream, S, A);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_render_graph_impl(const sdsm_set_image *images, int n_images, int n_prims, const int32_t *prims, double rim_radius,
                                             double disk_radius, int seed_reach, int line_reach, int core_d2, int ring_d2, const double *colors,
                                             const double *base, int channels, int32_t *key, uint8_t *out, hipStream_t stream)
{
    const RSet S = make_set(images, n_images, RTPB);
    GraphArgs A{};
    A.n_prims = n_prims; A.seed_reach = seed_reach; A.line_reach = line_reach; A.core_d2 = core_d2; A.ring_d2 = ring_d2; A.channels = channels;
    A.rim_radius = rim_radius; A.disk_radius = disk_radius;
    for (int k = 0; k < 12; k++) A.colors[k] = colors[k];
    A.prims = prims; A.base = base; A.key = key; A.out = out;
    for (int i = 0; i < n_images; i++) {
        hipError_t e = hipMemsetAsync(key + images[i].offset, 0, (size_t)images[i].H * images[i].W * sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
    }
    if (n_prims > 0) hipLaunchKernelGGL(k_graph_mark, dim3(n_prims), dim3(RTPB), 0, stream, S, A);
    hipLaunchKernelGGL(k_graph_paint, dim3(S.start[n_images]), dim3(RTPB), 0, stream, S, A);
    return hipGetLastError();
}
