// Image-wide steps of the coarse-to-fine region analysis (superdsm/c2freganal.py:110-126) on the GPU:
//
//   sdsm_c2f_markers   fg = y > 0, its 4-connected components (ndi.label), the P/A irregularity test of every component and the
//                      relabelled cluster markers (c2freganal.py:112-123), byte-equal to the SciPy statement.
//   sdsm_edt_exact     ndi.distance_transform_edt: exact squared distances in integers, then one correctly rounded sqrt.
//
// Labelling: union-find over the whole image.  A union hangs the larger of two roots under the smaller with atomicMin and retries
// if it lost a race, so parents only decrease and the root of a component is its minimum raster index whatever order the races
// resolve in.  Labels are the ranks of the roots in raster order (a prefix scan), which is the numbering ndi.label gives.
//
// Every phase is one launch for a whole set of images (the *_multi entry points; a single image is the set of one, sdsm_api.hip).  A
// workgroup (pixel blocks, scan chunks) or a thread (EDT columns and rows) finds its image in the prefix table of the launch, by binary
// search, and runs the __device__ body of its phase on pointers offset to the image, with pixel indices local to it.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/sdsm.h"
#include "sdsm_set.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK_PER_THREAD = 16;
constexpr int CHUNK = TPB * CHUNK_PER_THREAD;     // elements per block of the rank scan
constexpr int32_t EDT_INF = 0x7fffffff;

__device__ inline int find_root(const int32_t *P, int x)
{
    int p = __atomic_load_n(&P[x], __ATOMIC_RELAXED);
    while (p != x) {
        x = p;
        p = __atomic_load_n(&P[x], __ATOMIC_RELAXED);
    }
    return x;
}

__device__ inline void unite(int32_t *P, int a, int b)
{
    while (true) {
        a = find_root(P, a);
        b = find_root(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);       // a is a root: hang it under b unless somebody else re-parented it first
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ void markers_init(const double *y, int n, int p, int32_t *parent, int32_t *area, int32_t *bd, int32_t *n_bg)
{
    const bool inb = p < n;
    const bool fg = inb && y[p] > 0;                 // NaN is background, as in numpy
    if (inb) {
        parent[p] = fg ? p : -1;
        area[p] = 0;
        bd[p] = 0;
    }
    const int c = __syncthreads_count(inb && !fg);
    if (threadIdx.x == 0 && c) atomicAdd(n_bg, c);
}

__device__ __forceinline__ void markers_union(int H, int W, int p, int32_t *parent)
{
    if (p >= H * W || parent[p] < 0) return;
    const int r = p / W, c = p - r * W;
    if (c > 0 && parent[p - 1] >= 0) unite(parent, p, p - 1);
    if (r > 0 && parent[p - W] >= 0) unite(parent, p, p - W);
}

// after all unions: every pixel points at its root; area and boundary counts go to the root
__device__ __forceinline__ void markers_count(int H, int W, int p, int32_t *parent, int32_t *area, int32_t *bd)
{
    if (p >= H * W || parent[p] < 0) return;
    const int root = find_root(parent, p);
    const int r = p / W, c = p - r * W;
    // fg & ~binary_erosion(fg, disk(1)) with the border not eroding: some in-image 4-neighbour is background
    const bool boundary = (r > 0 && parent[p - W] < 0) || (r + 1 < H && parent[p + W] < 0) || (c > 0 && parent[p - 1] < 0) ||
                          (c + 1 < W && parent[p + 1] < 0);
    atomicAdd(&area[root], 1);
    if (boundary) atomicAdd(&bd[root], 1);
    parent[p] = root;                                 // safe: a root keeps parent == itself, others only move to their root
}

__device__ inline bool regular_root(const int32_t *parent, const int32_t *area, const int32_t *bd, int p, double thr)
{
    return parent[p] == p && !((double)bd[p] / (double)area[p] > thr);
}

__device__ inline int block_exclusive_scan(int v, int *total)
{
    __shared__ int s[TPB];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {
        const int t = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    const int incl = s[threadIdx.x];
    *total = s[TPB - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ int chunk_regular_count(int n, int chunk_index, const int32_t *parent, const int32_t *area, const int32_t *bd,
                                                   double thr)
{
    const int base = chunk_index * CHUNK + threadIdx.x * CHUNK_PER_THREAD;
    int cnt = 0;
    for (int k = 0; k < CHUNK_PER_THREAD; k++) {
        const int p = base + k;
        if (p < n && regular_root(parent, area, bd, p, thr)) cnt++;
    }
    return cnt;
}

__device__ __forceinline__ void markers_chunk_count(int n, int chunk_index, const int32_t *parent, const int32_t *area, const int32_t *bd,
                                                    double thr, int32_t *chunk)
{
    int total;
    block_exclusive_scan(chunk_regular_count(n, chunk_index, parent, area, bd, thr), &total);
    if (threadIdx.x == 0) chunk[chunk_index] = total;
}

// one block: exclusive scan of the chunk counts in place; the number of markers to d_count
__device__ __forceinline__ void markers_scan_chunks(int n_chunks, int32_t *chunk, const int32_t *n_bg, int32_t *d_count)
{
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_chunks; base += TPB) {
        const int i = base + threadIdx.x;
        const int v = i < n_chunks ? chunk[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        if (i < n_chunks) chunk[i] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    // no background pixel: the single component is relabelled 0 (_normalize_labels_map with label 0 absent)
    if (threadIdx.x == 0) *d_count = *n_bg > 0 ? carry : 0;
}

__device__ __forceinline__ void markers_rank(int n, int chunk_index, const int32_t *parent, const int32_t *area, const int32_t *bd, double thr,
                                             const int32_t *chunk, int32_t *lab)
{
    const int base = chunk_index * CHUNK + threadIdx.x * CHUNK_PER_THREAD;
    int total;
    int next = chunk[chunk_index] + block_exclusive_scan(chunk_regular_count(n, chunk_index, parent, area, bd, thr), &total) + 1;
    for (int k = 0; k < CHUNK_PER_THREAD; k++) {
        const int p = base + k;
        if (p < n && parent[p] == p) lab[p] = regular_root(parent, area, bd, p, thr) ? next++ : 0;
    }
}

__device__ __forceinline__ void markers_label(int n, int p, const int32_t *parent, const int32_t *lab, const int32_t *n_bg, double thr,
                                              uint8_t *y_mask, int32_t *markers)
{
    if (p >= n) return;
    const int root = parent[p];
    if (root < 0) {                                   // background: label 0, irregularity 0 / |background|
        y_mask[p] = !(0.0 > thr);
        markers[p] = 0;
        return;
    }
    const int l = lab[root];
    y_mask[p] = l > 0;
    markers[p] = *n_bg > 0 ? l : 0;
}

// ---- exact EDT -------------------------------------------------------------------------------------------------------------------

// one thread per column: row distance to the nearest target of the column (EDT_INF: none)
__device__ __forceinline__ void edt_col(const uint8_t *target, int H, int W, int c, int32_t *g)
{
    int last = -1;
    for (int r = 0; r < H; r++) {
        const size_t p = (size_t)r * W + c;
        if (target[p]) last = r;
        g[p] = last >= 0 ? r - last : EDT_INF;
    }
    last = -1;
    for (int r = H - 1; r >= 0; r--) {
        const size_t p = (size_t)r * W + c;
        if (target[p]) last = r;
        if (last >= 0 && last - r < g[p]) g[p] = last - r;
    }
}

// lower envelope of the parabolas (c - q)^2 + g(q)^2 of one row (Felzenszwalb & Huttenlocher), with the breakpoints compared as
// exact rationals in int64: s(p, q) = (f(q) + q^2 - f(p) - p^2) / (2 (q - p)) for p < q
__device__ inline int64_t edt_f(const int32_t *g, int q) { const int64_t v = g[q]; return v * v + (int64_t)q * q; }

__device__ __forceinline__ void edt_row(const int32_t *g, int W, int r, int32_t *v_ws, double *out)
{
    const int32_t *gr = g + (size_t)r * W;
    int32_t *v = v_ws + (size_t)r * W;
    double *o = out + (size_t)r * W;
    int k = -1;
    for (int q = 0; q < W; q++) {
        if (gr[q] == EDT_INF) continue;
        const int64_t fq = edt_f(gr, q);
        while (k >= 1) {
            // drop v[k] if s(v[k], q) <= s(v[k-1], v[k])
            const int a = v[k - 1], b = v[k];
            const int64_t fa = edt_f(gr, a), fb = edt_f(gr, b);
            const int64_t n1 = fq - fb, d1 = 2 * (int64_t)(q - b);
            const int64_t n2 = fb - fa, d2 = 2 * (int64_t)(b - a);
            if (n1 * d2 <= n2 * d1) k--;
            else break;
        }
        v[++k] = q;
    }
    if (k < 0) {                                      // no target at all: SciPy reports the distance to (-1, 0)
        for (int c = 0; c < W; c++) o[c] = sqrt((double)((int64_t)(r + 1) * (r + 1) + (int64_t)c * c));
        return;
    }
    int j = 0;
    for (int c = 0; c < W; c++) {
        // advance while s(v[j], v[j+1]) < c
        while (j < k) {
            const int a = v[j], b = v[j + 1];
            const int64_t num = edt_f(gr, b) - edt_f(gr, a), den = 2 * (int64_t)(b - a);
            if (num < (int64_t)c * den) j++;
            else break;
        }
        const int64_t dc = c - v[j], dr = gr[v[j]];
        o[c] = sqrt((double)(dc * dc + dr * dr));
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the kernels: one launch per phase and set ------------------------------------------------------------------------------------

// what the kernels of a set launch know about its images (a kernel argument, < 2 KB)
struct SetTable {
    int32_t n;
    int32_t H[SDSM_MAX_SET_IMAGES], W[SDSM_MAX_SET_IMAGES];
    int64_t off[SDSM_MAX_SET_IMAGES];            // element offset of the image in the caller's packed buffers
    int64_t woff[SDSM_MAX_SET_IMAGES];           // element offset of the image in the workspace's per-pixel arrays
    int64_t coff[SDSM_MAX_SET_IMAGES];           // offset of the image's scan chunks
    int32_t start[SDSM_MAX_SET_IMAGES + 1];      // prefix of the image's pixel blocks (markers) or columns (EDT)
    int32_t start2[SDSM_MAX_SET_IMAGES + 1];     // prefix of the image's scan chunks (markers) or rows (EDT)
    double thr[SDSM_MAX_SET_IMAGES];
};

__global__ void k_set_markers_init(SetTable T, const double *y, int32_t *parent, int32_t *area, int32_t *bd, int32_t *n_bg)
{
    const int i = set_find(T.start, T.n, blockIdx.x);
    const int64_t w = T.woff[i];
    markers_init(y + T.off[i], T.H[i] * T.W[i], (blockIdx.x - T.start[i]) * TPB + threadIdx.x, parent + w, area + w, bd + w, n_bg + i);
}

__global__ void k_set_markers_union(SetTable T, int32_t *parent)
{
    const int i = set_find(T.start, T.n, blockIdx.x);
    markers_union(T.H[i], T.W[i], (blockIdx.x - T.start[i]) * TPB + threadIdx.x, parent + T.woff[i]);
}

__global__ void k_set_markers_count(SetTable T, int32_t *parent, int32_t *area, int32_t *bd)
{
    const int i = set_find(T.start, T.n, blockIdx.x);
    const int64_t w = T.woff[i];
    markers_count(T.H[i], T.W[i], (blockIdx.x - T.start[i]) * TPB + threadIdx.x, parent + w, area + w, bd + w);
}

__global__ void k_set_markers_chunk_count(SetTable T, const int32_t *parent, const int32_t *area, const int32_t *bd, int32_t *chunk)
{
    const int i = set_find(T.start2, T.n, blockIdx.x);
    const int64_t w = T.woff[i];
    markers_chunk_count(T.H[i] * T.W[i], blockIdx.x - T.start2[i], parent + w, area + w, bd + w, T.thr[i], chunk + T.coff[i]);
}

// one block per image
__global__ void k_set_markers_scan_chunks(SetTable T, int32_t *chunk, const int32_t *n_bg, int32_t *d_count)
{
    const int i = blockIdx.x;
    markers_scan_chunks(T.start2[i + 1] - T.start2[i], chunk + T.coff[i], n_bg + i, d_count + i);
}

__global__ void k_set_markers_rank(SetTable T, const int32_t *parent, const int32_t *area, const int32_t *bd, const int32_t *chunk, int32_t *lab)
{
    const int i = set_find(T.start2, T.n, blockIdx.x);
    const int64_t w = T.woff[i];
    markers_rank(T.H[i] * T.W[i], blockIdx.x - T.start2[i], parent + w, area + w, bd + w, T.thr[i], chunk + T.coff[i], lab + w);
}

__global__ void k_set_markers_label(SetTable T, const int32_t *parent, const int32_t *lab, const int32_t *n_bg, uint8_t *y_mask, int32_t *markers)
{
    const int i = set_find(T.start, T.n, blockIdx.x);
    const int64_t w = T.woff[i];
    markers_label(T.H[i] * T.W[i], (blockIdx.x - T.start[i]) * TPB + threadIdx.x, parent + w, lab + w, n_bg + i, T.thr[i],
                  y_mask + T.off[i], markers + T.off[i]);
}

__global__ void k_set_edt_cols(SetTable T, const uint8_t *target, int32_t *g)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= T.start[T.n]) return;
    const int i = set_find(T.start, T.n, t);
    edt_col(target + T.off[i], T.H[i], T.W[i], t - T.start[i], g + T.woff[i]);
}

__global__ void k_set_edt_rows(SetTable T, const int32_t *g, int32_t *v_ws, double *out)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= T.start2[T.n]) return;
    const int i = set_find(T.start2, T.n, t);
    edt_row(g + T.woff[i], T.W[i], t - T.start2[i], v_ws + T.woff[i], out + T.off[i]);
}

// the table of a set and the sizes of its workspace arrays (in elements); edt: columns and rows instead of blocks and chunks
struct SetLayout {
    SetTable T;
    int64_t pixels, chunks;                      // elements of every per-pixel array, of the chunk array
};

SetLayout set_layout(const sdsm_set_image *im, int n, const double *thr, bool edt)
{
    SetLayout L{};
    L.T.n = n;
    L.T.start[0] = L.T.start2[0] = 0;
    for (int i = 0; i < n; i++) {
        const int64_t px = (int64_t)im[i].H * im[i].W;
        const int64_t chunks = (px + CHUNK - 1) / CHUNK;
        L.T.H[i] = im[i].H; L.T.W[i] = im[i].W; L.T.off[i] = im[i].offset;
        L.T.woff[i] = L.pixels; L.T.coff[i] = L.chunks;
        L.T.thr[i] = thr ? thr[i] : 0.0;
        L.T.start[i + 1] = L.T.start[i] + (int32_t)(edt ? im[i].W : (px + TPB - 1) / TPB);
        L.T.start2[i + 1] = L.T.start2[i] + (int32_t)(edt ? im[i].H : chunks);
        L.pixels += (px + 63) & ~(int64_t)63;    // every image's arrays start 256-byte aligned
        L.chunks += chunks;
    }
    return L;
}

}  // namespace

extern "C" size_t sdsm_c2f_markers_workspace_bytes_multi_impl(const sdsm_set_image *images, int n_images)
{
    const SetLayout L = set_layout(images, n_images, nullptr, false);
    return 4 * align256((size_t)L.pixels * 4) + align256((size_t)L.chunks * 4) + align256((size_t)n_images * 4);
}

extern "C" hipError_t sdsm_c2f_markers_multi_impl(const sdsm_set_image *images, int n_images, const double *d_y, const double *thr,
                                                  uint8_t *d_y_mask, int32_t *d_markers, int32_t *d_count, void *d_ws, hipStream_t stream)
{
    const SetLayout L = set_layout(images, n_images, thr, false);
    const SetTable &T = L.T;
    char *ws = (char *)d_ws;
    int32_t *parent = (int32_t *)ws; ws += align256((size_t)L.pixels * 4);
    int32_t *area = (int32_t *)ws; ws += align256((size_t)L.pixels * 4);
    int32_t *bd = (int32_t *)ws; ws += align256((size_t)L.pixels * 4);
    int32_t *lab = (int32_t *)ws; ws += align256((size_t)L.pixels * 4);
    int32_t *chunk = (int32_t *)ws; ws += align256((size_t)L.chunks * 4);
    int32_t *n_bg = (int32_t *)ws;
    hipError_t e = hipMemsetAsync(n_bg, 0, sizeof(int32_t) * n_images, stream);
    if (e != hipSuccess) return e;
    const int blocks = T.start[n_images], chunks = T.start2[n_images];
    hipLaunchKernelGGL(k_set_markers_init, dim3(blocks), dim3(TPB), 0, stream, T, d_y, parent, area, bd, n_bg);
    hipLaunchKernelGGL(k_set_markers_union, dim3(blocks), dim3(TPB), 0, stream, T, parent);
    hipLaunchKernelGGL(k_set_markers_count, dim3(blocks), dim3(TPB), 0, stream, T, parent, area, bd);
    hipLaunchKernelGGL(k_set_markers_chunk_count, dim3(chunks), dim3(TPB), 0, stream, T, parent, area, bd, chunk);
    hipLaunchKernelGGL(k_set_markers_scan_chunks, dim3(n_images), dim3(TPB), 0, stream, T, chunk, n_bg, d_count);
    hipLaunchKernelGGL(k_set_markers_rank, dim3(chunks), dim3(TPB), 0, stream, T, parent, area, bd, chunk, lab);
    hipLaunchKernelGGL(k_set_markers_label, dim3(blocks), dim3(TPB), 0, stream, T, parent, lab, n_bg, d_y_mask, d_markers);
    return hipGetLastError();
}

extern "C" size_t sdsm_edt_exact_workspace_bytes_multi_impl(const sdsm_set_image *images, int n_images)
{
    return 2 * align256((size_t)set_layout(images, n_images, nullptr, true).pixels * 4);
}

extern "C" hipError_t sdsm_edt_exact_multi_impl(const sdsm_set_image *images, int n_images, const uint8_t *d_target, double *d_out, void *d_ws,
                                                hipStream_t stream)
{
    const SetLayout L = set_layout(images, n_images, nullptr, true);
    int32_t *g = (int32_t *)d_ws;
    int32_t *v = (int32_t *)((char *)d_ws + align256((size_t)L.pixels * 4));
    const int cols = L.T.start[n_images], rows = L.T.start2[n_images];
    hipLaunchKernelGGL(k_set_edt_cols, dim3((cols + TPB - 1) / TPB), dim3(TPB), 0, stream, L.T, d_target, g);
    hipLaunchKernelGGL(k_set_edt_rows, dim3((rows + TPB - 1) / TPB), dim3(TPB), 0, stream, L.T, g, v, d_out);
    return hipGetLastError();
}
