// Connected parts of one label map on the GPU (superdsm_amd/parts.py): the part map (parts numbered by their first pixel in raster
// order), per label its parts, area, largest part and bit-quad counts, per part its label, area, first pixel and box, and the selection
// maps.  No reference counterpart; the definitions every kernel is tested against are parts_host and keep_maps_host.
//
//   k_parts_tiles   one workgroup per tile of PTH x PTW pixels of one image, on a flattened grid over the images of the set.
//       a. The tile and a halo of one place go to LDS as uint16; places outside the image and pixels with a label outside
//          0 .. n_labels - 1 are staged as 0 (the latter are counted in the image's status word), so nothing below tests a coordinate.
//       b. Union-find in LDS, parents as tile-local indices tr * PTW + tc.  A thread owns PSEG consecutive pixels of a tile row: the
//          pixels of a run of equal labels inside its segment start with the run's first pixel as parent, which costs no union.  Then
//          a pixel is united with its left neighbour at the start of a segment, and with the pixel above unless the pixel to its left
//          and the one above that carry the label too (they are united already, and so are the two above); under connectivity 8 with
//          the pixel above left and above right where the pixel above (or to the left) does not make the link.  The larger root hangs
//          under the smaller by an integer atomicMin; a thread that lost the race goes on from the parent it met, which is smaller.
//       c. The bit quads.  Window (i, j), 0 <= i <= H, 0 <= j <= W, has pixel (i, j) as its lower right place.  OWNERSHIP: it belongs to
//          the tile of pixel (min(i, H - 1), min(j, W - 1)), so the thread of pixel (r, c) counts window (r, c), and the windows
//          (r, W), (H, c), (H, W) where it is in the last column, the last row, or both.  A window that is not of one label is
//          classified per distinct label >= 1 (sdsm_parts_quad_inline); the counts of the current label stay in registers while it
//          does not change and go to an LDS table keyed by label on a change (lds_label_slot), which is flushed once per tile.  A
//          label that finds the slots taken goes straight to its global record.
//       d. Tile-local raster order is monotone in the image's raster order, so the local root is the tile's first pixel of the part:
//          every pixel gets the raster index of that pixel as its global parent (-1 on the background), by one plain store.
//   k_parts_seams   one thread per pixel beside a seam between two tiles: the pair across the seam, and under connectivity 8 the two
//       diagonal pairs across it (which covers the pairs across a tile corner from either seam).  Global unite by atomicMin on roots.
//   k_parts_flatten a thread owns PSEG consecutive pixels: each finds its root, stores it as its parent, and adds its run of pixels to
//       the root's area; the roots of the chunk are counted.
//   k_parts_scan    one workgroup per image: exclusive scan of the chunk counts; the total is K.
//   k_parts_rank    the roots of a chunk in raster order get chunk base + rank + 1: the part number goes to the part map at the root, and
//       the part to its label's record: n_parts and area by atomicAdd, the largest part by one 64-bit atomicMax of
//       area << 32 | (2^32 - 1 - part), so that of equal areas the smallest part number wins whatever the arrival order.
//   k_parts_map     every other pixel takes the part number from its root's place in the part map; 0 on the background.
//   k_parts_finish  largest_area and largest_part out of the label's key.
//   k_part_init, k_part_records   (sdsm_parts_table_multi) the part records, by atomicAdd / atomicMin / atomicMax per run of a part
//       along a row.
//   k_parts_keep    (sdsm_parts_keep_multi) the selection maps: two integer comparisons per pixel and selection.
//
// Every loop that retries ends because a parent strictly decreases: find walks down a chain of decreasing indices, and an iteration
// of unite either returns or goes on from a smaller index.  Nothing spins on a flag, no workgroup waits for another; the phases are
// separate launches on the caller's stream.  No float, no scratch.
#include <hip/hip_runtime.h>
#include "../../include/sdsm.h"
#include "sdsm_tables.h"
#include "sdsm_parts.h"

namespace {

constexpr int PTPB = 256;
constexpr int PTH = 32, PTW = 64;                // the tile: PTH rows of PTW pixels
constexpr int PSEG = 8;                          // consecutive pixels of a thread
constexpr int PCHUNK = PTPB * PSEG;              // pixels of a workgroup of the raster kernels
constexpr int PPITCH = PTW + 4;                  // staged labels per staged row: the tile, a halo of one, two places of padding
constexpr int PROWS = PTH + 2;
constexpr int PLBITS = 8;
constexpr int PLSLOTS = 1 << PLBITS;             // slots of the LDS label table (16 B each)
constexpr int PLPROBES = 8;                      //   slots tried before a label goes to the global records
static_assert(PTPB * PSEG == PTH * PTW && PTW % PSEG == 0 && PTW == 64, "a thread per segment covers the tile once; a wavefront per tile row");
static_assert(sizeof(sdsm_part_record) == 32 && sizeof(sdsm_part_label_record) == 32 && sizeof(sdsm_keep_spec) == 8, "record sizes of include/sdsm.h");

struct PSet {                                    // the images of a launch
    int32_t n, connectivity, n_keeps, pad;
    int32_t H[SDSM_MAX_SET_IMAGES], W[SDSM_MAX_SET_IMAGES], n_labels[SDSM_MAX_SET_IMAGES], n_parts[SDSM_MAX_SET_IMAGES];
    int32_t tiles_w[SDSM_MAX_SET_IMAGES];        // tiles per tile row
    int32_t start[SDSM_MAX_SET_IMAGES + 1];      // flattened grids: first tile of the image,
    int32_t start_seam[SDSM_MAX_SET_IMAGES + 1]; //   first workgroup of its seam pixels,
    int32_t start_chunk[SDSM_MAX_SET_IMAGES + 1];//   first chunk of PCHUNK pixels (and its place in the chunk counts)
    int64_t off[SDSM_MAX_SET_IMAGES];            // first pixel of the image in a packed buffer
    int64_t rec_off[SDSM_MAX_SET_IMAGES];        // first label record of the image
    int64_t part_off[SDSM_MAX_SET_IMAGES];       // first part record of the image
    int64_t keep_stride;                         // pixels from one selection's packed buffer to the next
    sdsm_keep_spec keep[SDSM_PARTS_MAX_KEEPS];
};
static_assert(sizeof(PSet) <= 4096, "passed by value");

struct PTile {
    int32_t parent[PTH * PTW];                   // tile-local index of the parent; a root is its own
    int32_t lkey[PLSLOTS];                       // -1: free
    uint32_t lval[3][PLSLOTS];                   // q1, q3, qd (a tile owns at most 33 * 65 windows)
    uint16_t lab[PROWS * PPITCH];                // staged place (rr, cc) is pixel (r0 - 1 + rr, c0 - 1 + cc)
};
static_assert(sizeof(PTile) <= 20 * 1024, "eight workgroups per compute unit");

// ---- union-find: in LDS (workgroup scope) and in global memory (agent scope) ---------------------------------------------------------
// parent[x] <= x always, so a walk ends; parents only decrease (atomicMin), so a root that was left stays left.
template <int SCOPE> __device__ __forceinline__ int uf_find(int32_t *parent, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        x = p;
    }
}

template <int SCOPE> __device__ __forceinline__ void uf_unite(int32_t *parent, int a, int b)
{
    for (;;) {
        a = uf_find<SCOPE>(parent, a);
        b = uf_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }        // a > b: a hangs under b
        const int old = atomicMin(parent + a, b);
        if (old == a) return;                    // a was a root still
        a = old;                                 // lost the race: old < a is (or was) a's parent; its tree and b's are joined next
    }
}

// ---- bit quads ---------------------------------------------------------------------------------------------------------------------
struct PQuads { int32_t label; uint32_t q1, q3, qd; };       // the counts the registers hold for `label`; label 0: none

__device__ __forceinline__ void quads_flush(PTile &T, sdsm_part_label_record *recs, const PQuads &n)
{
    if (n.label == 0) return;
    const int s = lds_label_slot<PLBITS, PLPROBES>(T.lkey, n.label);
    if (s >= 0) {
        if (n.q1) atomicAdd(&T.lval[0][s], n.q1);
        if (n.q3) atomicAdd(&T.lval[1][s], n.q3);
        if (n.qd) atomicAdd(&T.lval[2][s], n.qd);
    } else {                                     // no slot: correct and slow
        sdsm_part_label_record *rec = recs + n.label;
        if (n.q1) atomicAdd(&rec->q1, (int32_t)n.q1);
        if (n.q3) atomicAdd(&rec->q3, (int32_t)n.q3);
        if (n.qd) atomicAdd(&rec->qd, (int32_t)n.qd);
    }
}

__device__ __forceinline__ void quads_add(PTile &T, sdsm_part_label_record *recs, PQuads &n, int32_t a, int32_t b, int32_t c, int32_t d, int32_t label)
{
    const int k = sdsm_parts_quad_inline(a, b, c, d, label);
    if (k == SDSM_PARTS_QUAD_NONE) return;
    if (label != n.label) {
        quads_flush(T, recs, n);
        n.label = label; n.q1 = 0; n.q3 = 0; n.qd = 0;
    }
    n.q1 += k == SDSM_PARTS_QUAD_Q1;              // (three sums, not one counter picked by k: that would be an indexed array in scratch)
    n.q3 += k == SDSM_PARTS_QUAD_Q3;
    n.qd += k == SDSM_PARTS_QUAD_QD;
}

// the window whose lower right place is the staged place `at`: every distinct label >= 1 of its four places once
__device__ __forceinline__ void quads_window(PTile &T, sdsm_part_label_record *recs, PQuads &n, int at)
{
    const int32_t a = T.lab[at - PPITCH - 1], b = T.lab[at - PPITCH], c = T.lab[at - 1], d = T.lab[at];
    if (a == b && c == d && a == c) return;      // one label, or none: no class
    if (a) quads_add(T, recs, n, a, b, c, d, a);
    if (b && b != a) quads_add(T, recs, n, a, b, c, d, b);
    if (c && c != a && c != b) quads_add(T, recs, n, a, b, c, d, c);
    if (d && d != a && d != b && d != c) quads_add(T, recs, n, a, b, c, d, d);
}

// ---- the tiles -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PTPB) void k_parts_tiles(PSet S, const int32_t *labels_, sdsm_part_label_record *recs_, int32_t *parent_, int32_t *status_)
{
    __shared__ PTile T;
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int H = S.H[im], W = S.W[im], n_labels = S.n_labels[im];
    const int tile = blockIdx.x - S.start[im];
    const int r0 = (tile / S.tiles_w[im]) * PTH, c0 = (tile % S.tiles_w[im]) * PTW;
    const int32_t *lab = labels_ + S.off[im];
    sdsm_part_label_record *recs = recs_ + S.rec_off[im];
    const bool eight = S.connectivity == 8;

    // a. the label table, and the tile with its halo
    for (int s = tid; s < PLSLOTS; s += PTPB) { T.lkey[s] = -1; T.lval[0][s] = 0; T.lval[1][s] = 0; T.lval[2][s] = 0; }
    int n_bad = 0;
    for (int rr = tid >> 6; rr < PROWS; rr += PTPB / 64) {   // a wavefront per staged row: coalesced reads
        const int r = r0 - 1 + rr;
        const bool row_in = r >= 0 && r < H;
        for (int cc = tid & 63; cc < PTW + 2; cc += 64) {
            const int c = c0 - 1 + cc;
            int32_t l = 0;
            if (row_in && c >= 0 && c < W) {                 // (the only global reads: predicated)
                l = lab[(int64_t)r * W + c];
                if (l < 0 || l >= n_labels) {
                    l = 0;
                    if (rr >= 1 && rr <= PTH && cc >= 1 && cc <= PTW) n_bad++;       // counted by the tile that owns the pixel
                }
            }
            T.lab[rr * PPITCH + cc] = (uint16_t)l;
        }
    }
    if (n_bad) atomicAdd(status_ + im, n_bad);
    __syncthreads();

    // b. runs inside the segment: no union.  Pixel (tr, tc) is staged at (tr + 1) * PPITCH + tc + 1.
    const int tr = tid / (PTW / PSEG), tc0 = (tid % (PTW / PSEG)) * PSEG;
    {
        int run_start = 0;
        uint32_t prev = 0;
        for (int k = 0; k < PSEG; k++) {
            const int idx = tr * PTW + tc0 + k;
            const uint32_t l = T.lab[(tr + 1) * PPITCH + tc0 + k + 1];
            if (!(k > 0 && l != 0 && l == prev)) run_start = idx;
            T.parent[idx] = run_start;
            prev = l;
        }
    }
    __syncthreads();

    //    unions with the pixels of the tile to the left and above; the seams are k_parts_seams' (tr == 0, tc == 0, tc == PTW - 1 look
    //    at the halo only to decide, never to unite)
#pragma unroll 1
    for (int k = 0; k < PSEG; k++) {
        const int tc = tc0 + k, idx = tr * PTW + tc, at = (tr + 1) * PPITCH + tc + 1;
        const uint32_t l = T.lab[at];
        if (l == 0) continue;
        const bool left = tc > 0 && T.lab[at - 1] == l;
        if (k == 0 && left) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(T.parent, idx, idx - 1);
        if (tr == 0) continue;
        const bool up = T.lab[at - PPITCH] == l;
        if (up) {
            if (!(left && T.lab[at - PPITCH - 1] == l)) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(T.parent, idx, idx - PTW);
        } else if (eight) {
            if (tc > 0 && !left && T.lab[at - PPITCH - 1] == l) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(T.parent, idx, idx - PTW - 1);
            if (tc < PTW - 1 && T.lab[at - PPITCH + 1] == l) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(T.parent, idx, idx - PTW + 1);
        }
    }

    // c. the windows of the segment's pixels
    {
        PQuads n = {0, 0, 0, 0};
        const int r = r0 + tr;
        if (r < H) {
#pragma unroll 1
            for (int k = 0; k < PSEG; k++) {
                const int tc = tc0 + k, c = c0 + tc;
                if (c >= W) break;
                const int at = (tr + 1) * PPITCH + tc + 1;
                quads_window(T, recs, n, at);
                if (c == W - 1) quads_window(T, recs, n, at + 1);
                if (r == H - 1) {
                    quads_window(T, recs, n, at + PPITCH);
                    if (c == W - 1) quads_window(T, recs, n, at + PPITCH + 1);
                }
            }
        }
        quads_flush(T, recs, n);
    }
    __syncthreads();

    //    one lane per slot
    for (int s = tid; s < PLSLOTS; s += PTPB) {
        const int32_t label = T.lkey[s];
        if (label < 0) continue;
        sdsm_part_label_record *rec = recs + label;
        if (T.lval[0][s]) atomicAdd(&rec->q1, (int32_t)T.lval[0][s]);
        if (T.lval[1][s]) atomicAdd(&rec->q3, (int32_t)T.lval[1][s]);
        if (T.lval[2][s]) atomicAdd(&rec->qd, (int32_t)T.lval[2][s]);
    }

    // d. global parents, a wavefront per tile row
    int32_t *parent = parent_ + S.off[im];
    const int c = c0 + (tid & 63);
    if (c >= W) return;                          // (no barrier below)
    for (int row = tid >> 6; row < PTH; row += PTPB / 64) {
        const int r = r0 + row;
        if (r >= H) break;
        const int idx = row * PTW + (tid & 63);
        int32_t out = -1;
        if (T.lab[(row + 1) * PPITCH + (tid & 63) + 1]) {
            const int root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(T.parent, idx);
            out = (r0 + root / PTW) * W + c0 + root % PTW;   // < H * W < 2^30: the root is a pixel of the image
        }
        parent[(int64_t)r * W + c] = out;
    }
}

// ---- the seams -----------------------------------------------------------------------------------------------------------------------
// Image `im` has (tiles_w - 1) * H pixels left of a seam between tile columns, then (tiles_h - 1) * W above a seam between tile rows.
__global__ __launch_bounds__(PTPB) void k_parts_seams(PSet S, const int32_t *labels_, int32_t *parent_)
{
    const int im = set_find(S.start_seam, S.n, blockIdx.x);
    const int H = S.H[im], W = S.W[im];
    const int32_t *lab = labels_ + S.off[im];
    int32_t *parent = parent_ + S.off[im];
    const bool eight = S.connectivity == 8;
    int item = (blockIdx.x - S.start_seam[im]) * PTPB + threadIdx.x;
    const int n_right = (S.tiles_w[im] - 1) * H, n_down = ((H + PTH - 1) / PTH - 1) * W;
    // p and q are pixels of the image; a pixel with parent -1 is background (or out of range) and has no part
    auto pair = [&](int p, int q) {
        if (parent[p] < 0 || parent[q] < 0 || lab[p] != lab[q]) return;      // (-1 never changes, and no other parent becomes negative)
        uf_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, p, q);
    };
    if (item < n_right) {
        const int r = item % H, c = (item / H + 1) * PTW - 1;                // c + 1 < W: a tile column follows
        const int p = r * W + c;
        pair(p, p + 1);
        if (eight) {
            if (r + 1 < H) pair(p, p + W + 1);
            if (r >= 1) pair(p, p - W + 1);
        }
        return;
    }
    item -= n_right;
    if (item < n_down) {
        const int c = item % W, r = (item / W + 1) * PTH - 1;                // r + 1 < H: a tile row follows
        const int p = r * W + c;
        pair(p, p + W);
        if (eight) {
            if (c + 1 < W) pair(p, p + W + 1);
            if (c >= 1) pair(p, p + W - 1);
        }
    }
}

// ---- flatten, number, tables -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PTPB) void k_parts_flatten(PSet S, int32_t *parent_, int32_t *area_, int32_t *chunk)
{
    __shared__ int n_roots;
    const int im = set_find(S.start_chunk, S.n, blockIdx.x), tid = threadIdx.x;
    const int n = S.H[im] * S.W[im];
    int32_t *parent = parent_ + S.off[im], *area = area_ + S.off[im];
    if (tid == 0) n_roots = 0;
    __syncthreads();
    const int p0 = (blockIdx.x - S.start_chunk[im]) * PCHUNK + tid * PSEG;
    int roots = 0, run_root = -1, run_n = 0;
#pragma unroll 1
    for (int k = 0; k < PSEG; k++) {
        const int p = p0 + k;
        if (p >= n) break;
        const int par = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (par < 0) continue;
        const int root = uf_find<__HIP_MEMORY_SCOPE_AGENT>(parent, par);
        if (root != par) __hip_atomic_store(parent + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (an ancestor still: other walks stay right)
        roots += root == p;
        if (root != run_root) {
            if (run_n) atomicAdd(area + run_root, run_n);
            run_root = root;
            run_n = 0;
        }
        run_n++;
    }
    if (run_n) atomicAdd(area + run_root, run_n);
    if (roots) atomicAdd(&n_roots, roots);
    __syncthreads();
    if (tid == 0) chunk[blockIdx.x] = n_roots;
}

// exclusive scan over the workgroup; every thread calls it
__device__ __forceinline__ int block_exclusive_scan(int v, int *total, int *wave_sum)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    __syncthreads();                             // (the sums of an earlier call have been read)
    if (lane == 63) wave_sum[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < PTPB / 64; i++) {
        const int s = wave_sum[i];
        if (i < w) before += s;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(PTPB) void k_parts_scan(PSet S, int32_t *chunk_, int32_t *count)
{
    __shared__ int wave_sum[PTPB / 64];
    const int im = blockIdx.x, tid = threadIdx.x;
    int32_t *chunk = chunk_ + S.start_chunk[im];
    const int n_chunks = S.start_chunk[im + 1] - S.start_chunk[im];
    int carry = 0;
    for (int base = 0; base < n_chunks; base += PTPB) {      // (uniform: every thread makes every round)
        const int i = base + tid;
        const int v = i < n_chunks ? chunk[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total, wave_sum);
        if (i < n_chunks) chunk[i] = carry + ex;
        carry += total;
    }
    if (tid == 0) count[im] = carry;
}

__global__ __launch_bounds__(PTPB) void k_parts_rank(PSet S, const int32_t *labels_, const int32_t *parent_, const int32_t *area_, const int32_t *chunk,
                                                      sdsm_part_label_record *recs_, u64 *keys_, int32_t *part_map_)
{
    __shared__ int wave_sum[PTPB / 64];
    const int im = set_find(S.start_chunk, S.n, blockIdx.x), tid = threadIdx.x;
    const int n = S.H[im] * S.W[im];
    const int32_t *parent = parent_ + S.off[im], *area = area_ + S.off[im], *lab = labels_ + S.off[im];
    const int p0 = (blockIdx.x - S.start_chunk[im]) * PCHUNK + tid * PSEG;
    int roots = 0;
    for (int k = 0; k < PSEG; k++)
        if (p0 + k < n) roots += parent[p0 + k] == p0 + k;
    int total;
    int next = chunk[blockIdx.x] + block_exclusive_scan(roots, &total, wave_sum) + 1;
    if (!roots) return;                          // (no barrier below)
#pragma unroll 1
    for (int k = 0; k < PSEG; k++) {
        const int p = p0 + k;
        if (p >= n) break;
        if (parent[p] != p) continue;
        const int part = next++;
        part_map_[S.off[im] + p] = part;
        const int32_t l = lab[p], a = area[p];   // 1 <= l < n_labels: the tile kernel gave the pixel a parent
        sdsm_part_label_record *rec = recs_ + S.rec_off[im] + l;
        atomicAdd(&rec->n_parts, 1);
        atomicAdd(&rec->area, a);
        atomicMax(keys_ + S.rec_off[im] + l, ((u64)(uint32_t)a << 32) | (u64)(0xffffffffu - (uint32_t)part));
    }
}

__global__ __launch_bounds__(PTPB) void k_parts_map(PSet S, const int32_t *parent_, int32_t *part_map_)
{
    const int im = set_find(S.start_chunk, S.n, blockIdx.x);
    const int n = S.H[im] * S.W[im];
    const int32_t *parent = parent_ + S.off[im];
    int32_t *part_map = part_map_ + S.off[im];
    const int base = (blockIdx.x - S.start_chunk[im]) * PCHUNK + threadIdx.x;
    for (int k = 0; k < PSEG; k++) {
        const int p = base + k * PTPB;
        if (p >= n) break;
        const int root = parent[p];
        if (root == p) continue;                 // a root: k_parts_rank wrote it, and nobody else writes there
        part_map[p] = root < 0 ? 0 : part_map[root];
    }
}

__global__ __launch_bounds__(PTPB) void k_parts_finish(PSet S, sdsm_part_label_record *recs_, const u64 *keys_)
{
    const int im = blockIdx.y, l = blockIdx.x * PTPB + threadIdx.x;
    if (l >= S.n_labels[im]) return;
    const u64 key = keys_[S.rec_off[im] + l];
    if (key == 0) return;                        // no part: the record stays zero
    sdsm_part_label_record *rec = recs_ + S.rec_off[im] + l;
    rec->largest_area = (int32_t)(key >> 32);
    rec->largest_part = (int32_t)(0xffffffffu - (uint32_t)key);
}

// ---- the part table --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PTPB) void k_part_init(PSet S, sdsm_part_record *out_)
{
    const int im = blockIdx.y, k = blockIdx.x * PTPB + threadIdx.x;
    if (k >= S.n_parts[im]) return;
    out_[S.part_off[im] + k] = {0, 0, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0, 0, 0};
}

__device__ __forceinline__ void part_run(sdsm_part_record *rec, int32_t label, int first, int row, int col0, int col1, int n)
{
    atomicMax(&rec->label, label);
    atomicAdd(&rec->area, n);
    atomicMin(&rec->first, first);
    atomicMin(&rec->r0, row);
    atomicMax(&rec->r1, row + 1);
    atomicMin(&rec->c0, col0);
    atomicMax(&rec->c1, col1 + 1);
}

__global__ __launch_bounds__(PTPB) void k_part_records(PSet S, const int32_t *labels_, const int32_t *part_map_, sdsm_part_record *out_)
{
    const int im = set_find(S.start_chunk, S.n, blockIdx.x);
    const int W = S.W[im], n = S.H[im] * W, n_parts = S.n_parts[im];
    const int32_t *lab = labels_ + S.off[im], *part_map = part_map_ + S.off[im];
    sdsm_part_record *out = out_ + S.part_off[im];
    const int p0 = (blockIdx.x - S.start_chunk[im]) * PCHUNK + threadIdx.x * PSEG;
    if (p0 >= n) return;
    int row = p0 / W, col = p0 % W;
    int run_part = 0, run_first = 0, run_row = 0, run_col0 = 0, run_n = 0;   // the run of `run_part` along row run_row from run_col0 on; 0: none
    int32_t run_label = 0;
#pragma unroll 1
    for (int k = 0; k < PSEG && p0 + k < n; k++) {
        int part = part_map[p0 + k];
        if (part < 1 || part > n_parts) part = 0;
        if (part != run_part || row != run_row) {
            if (run_part) part_run(out + run_part - 1, run_label, run_first, run_row, run_col0, run_col0 + run_n - 1, run_n);
            run_part = part; run_first = p0 + k; run_row = row; run_col0 = col; run_n = 0;
            run_label = part ? lab[p0 + k] : 0;
        }
        run_n++;
        if (++col == W) { col = 0; row++; }
    }
    if (run_part) part_run(out + run_part - 1, run_label, run_first, run_row, run_col0, run_col0 + run_n - 1, run_n);
}

// ---- the selections ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PTPB) void k_parts_keep(PSet S, const int32_t *labels_, const int32_t *part_map_, const sdsm_part_label_record *recs_,
                                                      const sdsm_part_record *parts_, int32_t *out_)
{
    const int im = set_find(S.start_chunk, S.n, blockIdx.x);
    const int n = S.H[im] * S.W[im], n_labels = S.n_labels[im], n_parts = S.n_parts[im];
    const int base = (blockIdx.x - S.start_chunk[im]) * PCHUNK + threadIdx.x;
    for (int k = 0; k < PSEG; k++) {
        const int p = base + k * PTPB;
        if (p >= n) break;
        const int64_t px = S.off[im] + p;
        const int32_t l = labels_[px], part = part_map_[px];
        const bool ok = l >= 1 && l < n_labels && part >= 1 && part <= n_parts;
        const int32_t largest = ok ? recs_[S.rec_off[im] + l].largest_part : 0, area = ok ? parts_[S.part_off[im] + part - 1].area : 0;
        for (int z = 0; z < S.n_keeps; z++) {
            const sdsm_keep_spec &K = S.keep[z];
            int32_t v = 0;
            if (ok) {
                if (K.kind == SDSM_KEEP_SPLIT) v = part;
                else if (K.kind == SDSM_KEEP_LARGEST) v = part == largest ? l : 0;
                else v = area >= K.min_area ? l : 0;
            }
            out_[z * S.keep_stride + px] = v;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
PSet make_pset(const sdsm_set_image *images, int n_images)
{
    PSet S{};
    S.n = n_images;
    for (int i = 0; i < n_images; i++) {
        const int H = images[i].H, W = images[i].W;
        S.H[i] = H; S.W[i] = W; S.off[i] = images[i].offset;
        S.tiles_w[i] = (W + PTW - 1) / PTW;
        const int tiles_h = (H + PTH - 1) / PTH;
        S.start[i + 1] = S.start[i] + S.tiles_w[i] * tiles_h;
        const int64_t seam = (int64_t)(S.tiles_w[i] - 1) * H + (int64_t)(tiles_h - 1) * W;
        S.start_seam[i + 1] = S.start_seam[i] + (int32_t)((seam + PTPB - 1) / PTPB);
        S.start_chunk[i + 1] = S.start_chunk[i] + (int32_t)(((int64_t)H * W + PCHUNK - 1) / PCHUNK);
    }
    return S;
}

struct PWorkspace { size_t keys, parent, area, chunk, bytes; int64_t pixels, records; };

// keys (8 bytes per label record) first, then two int32 per pixel of the packed buffers, then the chunk counts
PWorkspace workspace(const sdsm_set_image *images, int n_images, const int64_t *rec_off, const int32_t *n_labels)
{
    PWorkspace w{};
    int64_t chunks = 0;
    for (int i = 0; i < n_images; i++) {
        const int64_t px = (int64_t)images[i].H * images[i].W;
        w.pixels = images[i].offset + px > w.pixels ? images[i].offset + px : w.pixels;
        w.records = rec_off[i] + n_labels[i] > w.records ? rec_off[i] + n_labels[i] : w.records;
        chunks += (px + PCHUNK - 1) / PCHUNK;
    }
    w.keys = 0;
    w.parent = (size_t)w.records * sizeof(u64);
    w.area = w.parent + (size_t)w.pixels * sizeof(int32_t);
    w.chunk = w.area + (size_t)w.pixels * sizeof(int32_t);
    w.bytes = w.chunk + (size_t)chunks * sizeof(int32_t);
    return w;
}

int max_of(const int32_t *v, int n)
{
    int m = 0;
    for (int i = 0; i < n; i++) m = v[i] > m ? v[i] : m;
    return m;
}

}  // namespace

extern "C" size_t sdsm_parts_workspace_bytes_impl(const sdsm_set_image *images, int n_images, const int64_t *rec_off, const int32_t *n_labels)
{
    return workspace(images, n_images, rec_off, n_labels).bytes;
}

// Cleared here, on the stream: the label records, the keys, the part areas and the status words.  Parents, chunk counts, K and the
// part map are written completely by the kernels.
extern "C" hipError_t sdsm_parts_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int connectivity, const int64_t *rec_off,
                                      const int32_t *n_labels, sdsm_part_label_record *d_label_out, int32_t *d_part_map, int32_t *d_count,
                                      int32_t *d_status, void *d_ws, hipStream_t stream)
{
    PSet S = make_pset(images, n_images);
    S.connectivity = connectivity;
    for (int i = 0; i < n_images; i++) { S.rec_off[i] = rec_off[i]; S.n_labels[i] = n_labels[i]; }
    const PWorkspace w = workspace(images, n_images, rec_off, n_labels);
    u64 *keys = (u64 *)((char *)d_ws + w.keys);
    int32_t *parent = (int32_t *)((char *)d_ws + w.parent), *area = (int32_t *)((char *)d_ws + w.area), *chunk = (int32_t *)((char *)d_ws + w.chunk);

    hipError_t e = hipSuccess;
    for (int i = 0; i < n_images && e == hipSuccess;) {
        int j = i + 1;
        while (j < n_images && rec_off[j] == rec_off[j - 1] + n_labels[j - 1]) j++;
        e = hipMemsetAsync(d_label_out + rec_off[i], 0, (size_t)(rec_off[j - 1] + n_labels[j - 1] - rec_off[i]) * sizeof(sdsm_part_label_record), stream);
        i = j;
    }
    if (e == hipSuccess) e = hipMemsetAsync(keys, 0, (size_t)w.records * sizeof(u64), stream);
    if (e == hipSuccess) e = hipMemsetAsync(area, 0, (size_t)w.pixels * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, (size_t)n_images * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;

    const int chunks = S.start_chunk[n_images];
    hipLaunchKernelGGL(k_parts_tiles, dim3(S.start[n_images]), dim3(PTPB), 0, stream, S, d_labels, d_label_out, parent, d_status);
    if (S.start_seam[n_images] > 0) hipLaunchKernelGGL(k_parts_seams, dim3(S.start_seam[n_images]), dim3(PTPB), 0, stream, S, d_labels, parent);
    hipLaunchKernelGGL(k_parts_flatten, dim3(chunks), dim3(PTPB), 0, stream, S, parent, area, chunk);
    hipLaunchKernelGGL(k_parts_scan, dim3(n_images), dim3(PTPB), 0, stream, S, chunk, d_count);
    hipLaunchKernelGGL(k_parts_rank, dim3(chunks), dim3(PTPB), 0, stream, S, d_labels, parent, area, chunk, d_label_out, keys, d_part_map);
    hipLaunchKernelGGL(k_parts_map, dim3(chunks), dim3(PTPB), 0, stream, S, parent, d_part_map);
    hipLaunchKernelGGL(k_parts_finish, dim3((max_of(n_labels, n_images) + PTPB - 1) / PTPB, n_images), dim3(PTPB), 0, stream, S, d_label_out, keys);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_parts_table_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map,
                                            const int64_t *part_off, const int32_t *n_parts, sdsm_part_record *d_part_out, hipStream_t stream)
{
    PSet S = make_pset(images, n_images);
    for (int i = 0; i < n_images; i++) { S.part_off[i] = part_off[i]; S.n_parts[i] = n_parts[i]; }
    const int most = max_of(n_parts, n_images);
    if (most == 0) return hipSuccess;            // no part in the set: nothing to write
    hipLaunchKernelGGL(k_part_init, dim3((most + PTPB - 1) / PTPB, n_images), dim3(PTPB), 0, stream, S, d_part_out);
    hipLaunchKernelGGL(k_part_records, dim3(S.start_chunk[n_images]), dim3(PTPB), 0, stream, S, d_labels, d_part_map, d_part_out);
    return hipGetLastError();
}

extern "C" hipError_t sdsm_parts_keep_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, const int32_t *d_part_map,
                                           const int64_t *rec_off, const int32_t *n_labels, const sdsm_part_label_record *d_label_recs,
                                           const int64_t *part_off, const int32_t *n_parts, const sdsm_part_record *d_part_recs, int n_keeps,
                                           const sdsm_keep_spec *keeps, int64_t keep_stride, int32_t *d_keep_out, hipStream_t stream)
{
    PSet S = make_pset(images, n_images);
    S.n_keeps = n_keeps;
    S.keep_stride = keep_stride;
    for (int z = 0; z < n_keeps; z++) S.keep[z] = keeps[z];
    for (int i = 0; i < n_images; i++) { S.rec_off[i] = rec_off[i]; S.n_labels[i] = n_labels[i]; S.part_off[i] = part_off[i]; S.n_parts[i] = n_parts[i]; }
    hipLaunchKernelGGL(k_parts_keep, dim3(S.start_chunk[n_images]), dim3(PTPB), 0, stream, S, d_labels, d_part_map, d_label_recs, d_part_recs, d_keep_out);
    return hipGetLastError();
}
