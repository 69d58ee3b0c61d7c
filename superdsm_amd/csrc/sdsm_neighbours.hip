// Neighbourhood tables of one label map on the GPU (superdsm_amd/neighbours.py): which labels lie within reach of each other, their
// smallest squared distance and the crack edges between them, and per label its pixels, boundary pixels, boundary pixels close to another
// label and pixel sides by what they face.  No reference counterpart; the definitions every kernel is tested against are
// neighbour_pairs_host and neighbour_labels_host.
//
//   k_neighbours<HALO>  one workgroup per tile of NTH x NTW pixels of one image.
//       1. The tile and a halo of reach = floor(sqrt(max_d2)) <= HALO pixels go to LDS as uint16; places outside the image and pixels with
//          a label outside 0 .. n_labels - 1 are staged as 0, so the search below never tests a coordinate.
//       2. A thread owns NSEG consecutive pixels of a tile row.  It reads their own labels from global memory again (a label out of range
//          is counted and skipped here), looks at the four sides of each and keeps the counts of its current label in registers while the
//          label does not change; on a change they go to an LDS table keyed by label.  A crack edge belongs to the pixel that has it on
//          its right or lower side, so each is counted once whatever the tiling.  Boundary pixels are appended to a list in LDS.
//       3. The boundary pixels are dealt to the lanes.  A lane walks the rows of the disk of its pixel by the half-width table; labels come
//          in runs along a row, so it keeps the current other label and its running minimum in registers and commits on a change, into
//          an LDS table keyed by the pair (64-bit LDS compare-and-swap, 32-bit min and add).  Only boundary pixels search: the closest pair
//          of pixels of two disjoint labels are boundary pixels of both (neighbours.py proves it, the tests pin it).
//       4. The occupied slots go to the label records (integer atomic adds) and to the image's global table (pair_table_slot of sdsm_tables.h,
//          atomicMin / atomicAdd on the two values).  A label or pair without an LDS slot goes straight there; a pair
//          without a global slot is counted and dropped, never waited for.
//
// Every atomic is an integer min, add or compare-and-swap, so the bytes (the pair table after a sort by key) do not depend on the order,
// the launch, the set size or the capacity.  No float, no scratch.
#include "sdsm_tables.h"
#include "sdsm_neighbours.h"

namespace {

constexpr int NTPB = 256;
constexpr int NTH = 32, NTW = 64;                // the tile: NTH rows of NTW pixels
constexpr int NSEG = 8;                          // consecutive pixels of a thread in phase 2: NTW / NSEG threads per tile row
constexpr int NPBITS = 8;
constexpr int NPSLOTS = 1 << NPBITS;             // slots of the LDS pair table (16 B each): a tile of nuclei meets a few dozen pairs
constexpr int NPPROBES = 8;                      //   slots tried before a pair goes to the global table
constexpr int NLBITS = 8;
constexpr int NLSLOTS = 1 << NLBITS;             // slots of the LDS label table (28 B each)
constexpr int NLPROBES = 8;                      //   slots tried before a label goes to the global records
constexpr int NFIELDS = 6;                       // area, boundary, close, edges_background, edges_labels, edges_frame
enum { F_AREA = 0, F_BOUNDARY, F_CLOSE, F_BACKGROUND, F_LABELS, F_FRAME };
static_assert(NTPB * NSEG == NTH * NTW && NTW % NSEG == 0, "phase 2 covers the tile once");
static_assert(sizeof(sdsm_neighbour_label) == 40 && sizeof(sdsm_neighbour_pair) == 16, "record sizes of include/sdsm.h");
static_assert(SDSM_NEIGHBOUR_MAX_D2 == SDSM_NEIGHBOUR_MAX_D2_INLINE && SDSM_NEIGHBOUR_MAX_REACH_INLINE * SDSM_NEIGHBOUR_MAX_REACH_INLINE == SDSM_NEIGHBOUR_MAX_D2,
              "the limit of the header and of the inline helpers");

struct NSet {                                    // the images of a launch
    int32_t n, max_d2, reach;
    int32_t H[SDSM_MAX_SET_IMAGES], W[SDSM_MAX_SET_IMAGES], n_labels[SDSM_MAX_SET_IMAGES];
    int32_t tiles_w[SDSM_MAX_SET_IMAGES];        // tiles per tile row
    int32_t start[SDSM_MAX_SET_IMAGES + 1];      // flattened grid: first workgroup of the image
    int64_t off[SDSM_MAX_SET_IMAGES];            // first pixel of the image in the packed buffer
    int64_t rec_off[SDSM_MAX_SET_IMAGES];        // first label record of the image
    int64_t table_off[SDSM_MAX_SET_IMAGES];      // first slot of the image's global table
    int64_t cap[SDSM_MAX_SET_IMAGES];            //   and its slots, a power of two
};

struct NGlobal {                                 // what a workgroup writes into: its image's part of every output
    sdsm_neighbour_label *recs;
    u64 *keys;
    uint32_t *min_d2, *contact;
    int64_t cap;
    int32_t *status;
};

template <int HALO> struct NTile {
    static constexpr int PITCH = NTW + 2 * HALO; // staged labels per staged row
    static constexpr int ROWS = NTH + 2 * HALO;
    u64 pkey[NPSLOTS];                           // PAIR_FREE: free
    uint32_t pmin[NPSLOTS], pcnt[NPSLOTS];
    int32_t lkey[NLSLOTS];                       // -1: free
    uint32_t lval[NFIELDS][NLSLOTS];             // (a tile has 2048 pixels and 8192 sides)
    int32_t n_list;
    uint16_t list[NTH * NTW];                    // boundary pixels of the tile, row * NTW + column, in arrival order
    int16_t hw[2 * HALO + 1];                    // half-width of row d_row of the disk at [d_row + reach]
    uint16_t lab[ROWS * PITCH];                  // staged place (rr, cc) is pixel (r0 - reach + rr, c0 - reach + cc)
};
static_assert(sizeof(NTile<64>) <= 80 * 1024, "two workgroups per compute unit at the largest halo");

// d2 / contact of the pair `key` into the global table of its image (pair_table_slot, from sdsm_neighbour_slot on); a pair that finds the
// table full is counted in status[1] and dropped
__device__ __forceinline__ void pair_global(const NGlobal &G, u64 key, uint32_t d2, uint32_t contact)
{
    const bool found = pair_table_slot(G.keys, G.cap, sdsm_neighbour_slot_inline(key, (u64)G.cap), key, [&](u64 s) {
        atomicMin(G.min_d2 + s, d2);
        if (contact) atomicAdd(G.contact + s, contact);
    });
    if (!found) atomicAdd(G.status + 1, 1);
}

template <class Tile> __device__ __forceinline__ void pair_commit(Tile &T, const NGlobal &G, uint32_t l, uint32_t other, uint32_t d2, uint32_t contact)
{
    const u64 key = l < other ? ((u64)l << 32) | other : ((u64)other << 32) | l;
    uint32_t s = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - NPBITS));
    for (int k = 0; k < NPPROBES; k++, s = (s + 1) & (NPSLOTS - 1)) {
        const u64 old = atomicCAS(&T.pkey[s], PAIR_FREE, key);
        if (old != PAIR_FREE && old != key) continue;
        atomicMin(&T.pmin[s], d2);
        if (contact) atomicAdd(&T.pcnt[s], contact);
        return;
    }
    pair_global(G, key, d2, contact);            // no slot: correct and slow
}

__device__ __forceinline__ void label_global(sdsm_neighbour_label *rec, int field, uint32_t v)
{
    if (field == F_AREA) atomicAdd(&rec->area, (int32_t)v);
    else if (field == F_BOUNDARY) atomicAdd(&rec->boundary, (int32_t)v);
    else if (field == F_CLOSE) atomicAdd(&rec->close, (int32_t)v);
    else if (field == F_BACKGROUND) atomicAdd((u64 *)&rec->edges_background, (u64)v);
    else if (field == F_LABELS) atomicAdd((u64 *)&rec->edges_labels, (u64)v);
    else atomicAdd((u64 *)&rec->edges_frame, (u64)v);
}

template <class Tile> __device__ __forceinline__ void label_add(Tile &T, const NGlobal &G, int32_t label, int field, uint32_t v)
{
    const int s = lds_label_slot<NLBITS, NLPROBES>(T.lkey, label);
    if (s >= 0) atomicAdd(&T.lval[field][s], v);
    else label_global(G.recs + label, field, v);             // no slot: correct and slow
}

struct NCounts { uint32_t area, boundary, background, labels, frame; };

template <class Tile> __device__ __forceinline__ void counts_flush(Tile &T, const NGlobal &G, int32_t label, const NCounts &c)
{
    const int s = lds_label_slot<NLBITS, NLPROBES>(T.lkey, label);
    if (s >= 0) {
        atomicAdd(&T.lval[F_AREA][s], c.area);
        if (c.boundary) atomicAdd(&T.lval[F_BOUNDARY][s], c.boundary);
        if (c.background) atomicAdd(&T.lval[F_BACKGROUND][s], c.background);
        if (c.labels) atomicAdd(&T.lval[F_LABELS][s], c.labels);
        if (c.frame) atomicAdd(&T.lval[F_FRAME][s], c.frame);
    } else {
        sdsm_neighbour_label *rec = G.recs + label;
        label_global(rec, F_AREA, c.area);
        if (c.boundary) label_global(rec, F_BOUNDARY, c.boundary);
        if (c.background) label_global(rec, F_BACKGROUND, c.background);
        if (c.labels) label_global(rec, F_LABELS, c.labels);
        if (c.frame) label_global(rec, F_FRAME, c.frame);
    }
}

template <int HALO> __global__ __launch_bounds__(NTPB) void k_neighbours(NSet S, const int32_t *labels_, sdsm_neighbour_label *recs_, u64 *keys_,
                                                                           uint32_t *min_d2_, uint32_t *contact_, int32_t *status_)
{
    typedef NTile<HALO> Tile;
    __shared__ Tile T;
    constexpr int PITCH = Tile::PITCH;
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int H = S.H[im], W = S.W[im], n_labels = S.n_labels[im], R = S.reach;      // R <= HALO: the host chose the instance
    if (R < 1 || R > HALO) return;               // (never: every index below relies on it)
    const int tile = blockIdx.x - S.start[im];
    const int r0 = (tile / S.tiles_w[im]) * NTH, c0 = (tile % S.tiles_w[im]) * NTW;
    const int32_t *lab = labels_ + S.off[im];
    const NGlobal G = {recs_ + S.rec_off[im], keys_ + S.table_off[im], min_d2_ + S.table_off[im], contact_ + S.table_off[im], S.cap[im], status_ + 2 * im};

    // 1. tables, and the tile with its halo.  Staged rows NTH + 2 R, staged columns NTW + 2 R: inside ROWS x PITCH as R <= HALO.
    for (int s = tid; s < NPSLOTS; s += NTPB) { T.pkey[s] = PAIR_FREE; T.pmin[s] = 0xffffffffu; T.pcnt[s] = 0; }
    for (int s = tid; s < NLSLOTS; s += NTPB) {
        T.lkey[s] = -1;
        for (int f = 0; f < NFIELDS; f++) T.lval[f][s] = 0;
    }
    if (tid <= 2 * R) T.hw[tid] = (int16_t)sdsm_neighbour_halfwidth_inline(S.max_d2, tid - R);
    if (tid == 0) T.n_list = 0;
    const int rows = NTH + 2 * R, cols = NTW + 2 * R;
    for (int rr = tid >> 6; rr < rows; rr += NTPB / 64) {    // a wavefront per staged row: coalesced reads
        const int r = r0 - R + rr;
        const bool row_in = r >= 0 && r < H;
        for (int cc = tid & 63; cc < cols; cc += 64) {
            const int c = c0 - R + cc;
            int32_t l = 0;
            if (row_in && c >= 0 && c < W) {                 // (the only global reads of the map besides phase 2's: both predicated)
                l = lab[(int64_t)r * W + c];
                if (l < 0 || l >= n_labels) l = 0;
            }
            T.lab[rr * PITCH + cc] = (uint16_t)l;
        }
    }
    __syncthreads();

    // 2. own pixels: NSEG consecutive pixels of tile row tr
    {
        const int tr = tid / (NTW / NSEG), tc0 = (tid % (NTW / NSEG)) * NSEG;
        const int r = r0 + tr;
        int32_t cur = -1;                        // the label whose counts the registers hold; -1: none
        NCounts n = {0, 0, 0, 0, 0};
        int n_bad = 0;
        if (r < H) {
#pragma unroll 1
            for (int k = 0; k < NSEG; k++) {     // (one flush site: the loop stays rolled)
                const int tc = tc0 + k, c = c0 + tc;
                if (c >= W) break;
                const int32_t l = lab[(int64_t)r * W + c];
                if (l < 0 || l >= n_labels) { n_bad++; continue; }       // skipped; the run of the current label goes on behind it
                if (l != cur) {
                    if (cur >= 0) counts_flush(T, G, cur, n);
                    cur = l;
                    n = {0, 0, 0, 0, 0};
                }
                n.area++;
                if (l == 0) continue;
                const int at = (tr + R) * PITCH + (tc + R);  // this pixel among the staged ones
                bool edge = false;
                // up, left: sides that the other pixel owns
                if (r == 0) n.frame++;
                else { const int32_t o = T.lab[at - PITCH]; if (o != l) { edge = true; if (o) n.labels++; else n.background++; } }
                if (c == 0) n.frame++;
                else { const int32_t o = T.lab[at - 1]; if (o != l) { edge = true; if (o) n.labels++; else n.background++; } }
                // down, right: sides that this pixel owns
                if (r + 1 == H) n.frame++;
                else {
                    const int32_t o = T.lab[at + PITCH];
                    if (o != l) { edge = true; if (o) { n.labels++; pair_commit(T, G, (uint32_t)l, (uint32_t)o, 1u, 1u); } else n.background++; }
                }
                if (c + 1 == W) n.frame++;
                else {
                    const int32_t o = T.lab[at + 1];
                    if (o != l) { edge = true; if (o) { n.labels++; pair_commit(T, G, (uint32_t)l, (uint32_t)o, 1u, 1u); } else n.background++; }
                }
                if (edge) {
                    n.boundary++;
                    T.list[atomicAdd(&T.n_list, 1)] = (uint16_t)(tr * NTW + tc);     // (at most NTH * NTW appends: one per pixel)
                }
            }
            if (cur >= 0) counts_flush(T, G, cur, n);
        }
        if (n_bad) atomicAdd(G.status, n_bad);
    }
    __syncthreads();

    // 3. the disk of every boundary pixel.  Staged row tr + R + d_row lies in 0 .. NTH + 2 R - 1 and staged column tc + R + d_col in
    //    0 .. NTW + 2 R - 1 for |d_row|, |d_col| <= R: every read is one of a staged place.
    const int n_list = T.n_list;
    for (int i = tid; i < n_list; i += NTPB) {
        const int p = T.list[i], tr = p / NTW, tc = p % NTW;
        const int at = (tr + R) * PITCH + (tc + R);
        const uint32_t l = T.lab[at];
        uint32_t other = 0, best = 0;            // the label of the current run of other labels and its smallest d2; 0: none
        bool found = false;
#pragma unroll 1
        for (int dr = -R; dr <= R; dr++) {
            const int w = T.hw[dr + R];          // >= 0: dr * dr <= R * R <= max_d2
            const uint16_t *row = T.lab + at + dr * PITCH;
            const uint32_t rr2 = (uint32_t)(dr * dr);
#pragma unroll 1
            for (int dc = -w; dc <= w; dc++) {
                const uint32_t o = row[dc];
                if (o == 0 || o == l) continue;
                const uint32_t d2 = rr2 + (uint32_t)(dc * dc);
                if (o == other) { best = d2 < best ? d2 : best; continue; }
                if (other) pair_commit(T, G, l, other, best, 0u);
                other = o;
                best = d2;
                found = true;
            }
        }
        if (other) pair_commit(T, G, l, other, best, 0u);
        if (found) label_add(T, G, (int32_t)l, F_CLOSE, 1u);
    }
    __syncthreads();

    // 4. one lane per slot
    for (int s = tid; s < NPSLOTS; s += NTPB)
        if (T.pkey[s] != PAIR_FREE) pair_global(G, T.pkey[s], T.pmin[s], T.pcnt[s]);
    for (int s = tid; s < NLSLOTS; s += NTPB) {
        const int32_t label = T.lkey[s];
        if (label < 0) continue;
        sdsm_neighbour_label *rec = G.recs + label;
        for (int f = 0; f < NFIELDS; f++)
            if (T.lval[f][s]) label_global(rec, f, T.lval[f][s]);
    }
}

template <int HALO> void launch(const NSet &S, const int32_t *labels, sdsm_neighbour_label *recs, uint64_t *keys, uint32_t *min_d2, uint32_t *contact,
                                int32_t *status, hipStream_t stream)
{
    hipLaunchKernelGGL(k_neighbours<HALO>, dim3(S.start[S.n]), dim3(NTPB), 0, stream, S, labels, recs, (u64 *)keys, min_d2, contact, status);
}

}  // namespace

// The outputs are cleared here, on the stream: records, contact counts and status to 0, keys and minima to bytes 0xFF; ranges of images
// that follow each other in the buffers are cleared by one call.
extern "C" hipError_t sdsm_neighbours_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, const int64_t *rec_off,
                                           const int32_t *n_labels, sdsm_neighbour_label *d_label_out, const int64_t *table_off,
                                           const int64_t *capacity, uint64_t *d_keys, uint32_t *d_min_d2, uint32_t *d_contact, int32_t *d_status,
                                           hipStream_t stream)
{
    NSet S{};
    S.n = n_images;
    S.max_d2 = max_d2;
    S.reach = sdsm_neighbour_isqrt_inline(max_d2);
    for (int i = 0; i < n_images; i++) {
        S.H[i] = images[i].H; S.W[i] = images[i].W; S.off[i] = images[i].offset;
        S.n_labels[i] = n_labels[i]; S.rec_off[i] = rec_off[i]; S.table_off[i] = table_off[i]; S.cap[i] = capacity[i];
        S.tiles_w[i] = (images[i].W + NTW - 1) / NTW;
        S.start[i + 1] = S.start[i] + S.tiles_w[i] * ((images[i].H + NTH - 1) / NTH);
    }
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_images && e == hipSuccess;) {
        int j = i + 1;
        while (j < n_images && rec_off[j] == rec_off[j - 1] + n_labels[j - 1]) j++;
        e = hipMemsetAsync(d_label_out + rec_off[i], 0, (size_t)(rec_off[j - 1] + n_labels[j - 1] - rec_off[i]) * sizeof(sdsm_neighbour_label), stream);
        i = j;
    }
    for (int i = 0; i < n_images && e == hipSuccess;) {
        int j = i + 1;
        while (j < n_images && table_off[j] == table_off[j - 1] + capacity[j - 1]) j++;
        const size_t first = (size_t)table_off[i], slots = (size_t)(table_off[j - 1] + capacity[j - 1] - table_off[i]);
        e = hipMemsetAsync(d_keys + first, 0xFF, slots * sizeof(uint64_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_min_d2 + first, 0xFF, slots * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_contact + first, 0, slots * sizeof(uint32_t), stream);
        i = j;
    }
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, (size_t)n_images * 2 * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (S.reach <= 4) launch<4>(S, d_labels, d_label_out, d_keys, d_min_d2, d_contact, d_status, stream);
    else if (S.reach <= 16) launch<16>(S, d_labels, d_label_out, d_keys, d_min_d2, d_contact, d_status, stream);
    else launch<64>(S, d_labels, d_label_out, d_keys, d_min_d2, d_contact, d_status, stream);
    return hipGetLastError();
}
