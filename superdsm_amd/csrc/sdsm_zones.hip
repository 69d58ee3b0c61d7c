// Zone label maps of one label map on the GPU (superdsm_amd/zones.py): per pixel the nearest place within reach that carries another
// label -- its squared distance and that label --, and from the two the zone maps: the labels grown into the background, the band
// around them, their cores and their rims.  No reference counterpart; the definitions every kernel is tested against are
// nearest_other_host and zone_maps_host.
//
//   k_zones<HALO>  one workgroup per tile of ZTH x ZTW pixels of one image, on a flattened grid over the images of the set.
//       a. The tile and a halo of reach = floor(sqrt(max_d2)) <= HALO pixels go to LDS as uint16; places outside the image and pixels
//          with a label outside 0 .. 65535 are staged as 0 (the latter are counted in the image's status word), so nothing below tests a
//          coordinate.
//       b. One thread per staged column walks it down and then up and leaves, for every tile row, the vertical distance to the first
//          place above and below whose label differs from the label at that place, capped at reach + 1 ("none within reach"), as two
//          bytes of one uint16.  A run that leaves the staged rows is longer than the reach of every tile row, so the cap is exact.
//       c. A thread owns one column of the tile and every fourth row.  For its pixel p = (r, c) it scans the staged places (r, c') by
//          growing |c' - c|: a place with another label is the candidate (dc^2, label); a place with the label of p stands for its column
//          by its two run ends, (dc^2 + up^2, label above) and (dc^2 + down^2, label below), each only within max_d2 -- if the place
//          carries L(p), the nearest place of its column that differs from L(p) is a run end.  The smallest key d2 << 16 | label is
//          kept, and the scan ends when dc^2 exceeds the best d2: nothing further out can win or tie.
//          The maps are written from registers: d2, other (either only if asked for) and one map per zone.
//
// Lanes of a wavefront hold consecutive columns of one row, so the row scan reads consecutive uint16 (two lanes share a bank word and
// read the same address), the run bytes likewise, and every global store is a full row segment.  The column walks of (b) read one
// staged row per step, consecutive columns across the lanes.  Only the reads of the label at a run end go to differing rows; the
// staged pitch is a multiple of four bank words at every halo class.  No float, no atomic on a map, no scratch.
#include <hip/hip_runtime.h>
#include "../../include/sdsm.h"
#include "sdsm_set.h"
#include "sdsm_neighbours.h"

namespace {

constexpr int ZTPB = 256;
constexpr int ZTH = 32, ZTW = 64;                // the tile: ZTH rows of ZTW pixels, a wavefront per row
constexpr uint32_t Z_NONE = 0xffffffffu;         // the key of "nothing found"
static_assert(ZTW == 64 && ZTPB % ZTW == 0 && ZTH % (ZTPB / ZTW) == 0, "a wavefront per tile row, every row once");
static_assert(sizeof(sdsm_zone_spec) == 16, "record size of include/sdsm.h");
static_assert(SDSM_ZONE_MAX_D2 == SDSM_NEIGHBOUR_MAX_D2_INLINE, "the integer root of sdsm_neighbours.h covers the reach");
static_assert(SDSM_ZONE_NO_UPPER == 0x7fffffff, "an unbounded zone and a pixel without a nearest place compare as equal");

struct ZSet {                                    // the images and the zones of a launch
    int32_t n, max_d2, reach, n_zones;
    int32_t H[SDSM_MAX_SET_IMAGES], W[SDSM_MAX_SET_IMAGES];
    int32_t tiles_w[SDSM_MAX_SET_IMAGES];        // tiles per tile row
    int32_t start[SDSM_MAX_SET_IMAGES + 1];      // flattened grid: first workgroup of the image
    int64_t off[SDSM_MAX_SET_IMAGES];            // first pixel of the image in a packed buffer
    int64_t zone_stride;                         // pixels from one zone's packed buffer to the next
    sdsm_zone_spec zone[SDSM_ZONE_MAX_ZONES];
};

template <int HALO> struct ZTile {
    static constexpr int PITCH = ZTW + 2 * HALO; // staged labels per staged row
    static constexpr int ROWS = ZTH + 2 * HALO;
    uint16_t lab[ROWS * PITCH];                  // staged place (rr, cc) is pixel (r0 - reach + rr, c0 - reach + cc)
    uint16_t run[ZTH * PITCH];                   // tile row tr, staged column cc: up | down << 8, each 1 .. reach + 1
};
static_assert(sizeof(ZTile<64>) <= 80 * 1024, "two workgroups per compute unit at the largest halo");
static_assert(ZTile<4>::PITCH % 8 == 0 && ZTile<16>::PITCH % 8 == 0 && ZTile<64>::PITCH % 8 == 0, "staged rows start on a multiple of four bank words");

// the candidates that the staged place `at` of tile row tr, staged column cc, stands for when it carries the label of the pixel: the
// ends of its run up and down the column, dc2 to the side.  up, down <= R read a staged row: at - up * PITCH is row tr + R - up >= 0.
template <class Tile> __device__ __forceinline__ uint32_t run_ends(const Tile &T, int at, int run_at, uint32_t dc2, int R, uint32_t max_d2, uint32_t best)
{
    const uint32_t rn = T.run[run_at], up = rn & 0xffu, down = rn >> 8;
    if ((int)up <= R) {
        const uint32_t d2 = dc2 + up * up;
        if (d2 <= max_d2) { const uint32_t key = (d2 << 16) | T.lab[at - (int)up * Tile::PITCH]; best = key < best ? key : best; }
    }
    if ((int)down <= R) {
        const uint32_t d2 = dc2 + down * down;
        if (d2 <= max_d2) { const uint32_t key = (d2 << 16) | T.lab[at + (int)down * Tile::PITCH]; best = key < best ? key : best; }
    }
    return best;
}

template <int HALO> __global__ __launch_bounds__(ZTPB) void k_zones(ZSet S, const int32_t *labels_, int32_t *d2_out_, int32_t *other_out_, int32_t *zone_out_,
                                                                     int32_t *status_)
{
    typedef ZTile<HALO> Tile;
    __shared__ Tile T;
    constexpr int PITCH = Tile::PITCH;
    const int im = set_find(S.start, S.n, blockIdx.x), tid = threadIdx.x;
    const int H = S.H[im], W = S.W[im], R = S.reach;         // R <= HALO: the host chose the instance
    if (R < 1 || R > HALO) return;               // (never: every index below relies on it)
    const int tile = blockIdx.x - S.start[im];
    const int r0 = (tile / S.tiles_w[im]) * ZTH, c0 = (tile % S.tiles_w[im]) * ZTW;
    const int32_t *lab = labels_ + S.off[im];
    const uint32_t max_d2 = (uint32_t)S.max_d2;

    // a. the tile with its halo.  Staged rows ZTH + 2 R, staged columns ZTW + 2 R: inside ROWS x PITCH as R <= HALO.
    const int rows = ZTH + 2 * R, cols = ZTW + 2 * R;
    int n_bad = 0;
    for (int rr = tid >> 6; rr < rows; rr += ZTPB / 64) {    // a wavefront per staged row: coalesced reads
        const int r = r0 - R + rr;
        const bool row_in = r >= 0 && r < H;
        for (int cc = tid & 63; cc < cols; cc += 64) {
            const int c = c0 - R + cc;
            int32_t l = 0;
            if (row_in && c >= 0 && c < W) {                 // (the only global reads: predicated)
                l = lab[(int64_t)r * W + c];
                if (l < 0 || l >= SDSM_BOUNDARY_MAX_LABELS) {
                    l = 0;
                    if (rr >= R && rr < R + ZTH && cc >= R && cc < R + ZTW) n_bad++;     // counted by the tile that owns the pixel
                }
            }
            T.lab[rr * PITCH + cc] = (uint16_t)l;
        }
    }
    if (n_bad) atomicAdd(status_ + im, n_bad);
    __syncthreads();

    // b. runs.  Walking down, `run` is the distance from staged row rr up to the first place with another label; a place above staged row
    //    0 is taken to differ, which gives rr + 1 >= R + 1 for a tile row (rr >= R): beyond reach, as it is.  Walking up likewise from the
    //    last staged row, ZTH + 2 R - 1 >= R + ZTH.  Tile rows are the staged rows R .. R + ZTH - 1.
    for (int cc = tid; cc < cols; cc += ZTPB) {
        uint32_t prev = T.lab[cc], run = 1;
        for (int rr = 1; rr < R + ZTH; rr++) {
            const uint32_t cur = T.lab[rr * PITCH + cc];
            run = cur == prev ? run + 1 : 1;
            prev = cur;
            if (rr >= R) T.run[(rr - R) * PITCH + cc] = (uint16_t)(run > (uint32_t)R ? R + 1 : run);
        }
        prev = T.lab[(rows - 1) * PITCH + cc];
        run = 1;
        for (int rr = rows - 2; rr >= R; rr--) {
            const uint32_t cur = T.lab[rr * PITCH + cc];
            run = cur == prev ? run + 1 : 1;
            prev = cur;
            if (rr < R + ZTH) T.run[(rr - R) * PITCH + cc] |= (uint16_t)((run > (uint32_t)R ? R + 1 : run) << 8);   // (this thread wrote the low byte)
        }
    }
    __syncthreads();

    // c. pixels.  Staged column tc + R + dc lies in 0 .. ZTW + 2 R - 1 for |dc| <= R: every read is one of a staged place.
    const int tc = tid & (ZTW - 1), c = c0 + tc;
    if (c >= W) return;                          // (no barrier below)
    const int64_t stride = S.zone_stride;
#pragma unroll 1
    for (int tr = tid / ZTW; tr < ZTH; tr += ZTPB / ZTW) {
        const int r = r0 + tr;
        if (r >= H) break;
        const int at = (tr + R) * PITCH + (tc + R), run_at = tr * PITCH + (tc + R);
        const uint32_t l = T.lab[at];
        uint32_t best = run_ends(T, at, run_at, 0u, R, max_d2, Z_NONE);
#pragma unroll 1
        for (int a = 1; a <= R; a++) {
            const uint32_t dc2 = (uint32_t)(a * a);
            if (dc2 > (best >> 16)) break;       // (Z_NONE >> 16 = 65535 > R * R)
            const uint32_t left = T.lab[at - a], right = T.lab[at + a];
            if (left != l) { const uint32_t key = (dc2 << 16) | left; best = key < best ? key : best; }
            else best = run_ends(T, at - a, run_at - a, dc2, R, max_d2, best);
            if (right != l) { const uint32_t key = (dc2 << 16) | right; best = key < best ? key : best; }
            else best = run_ends(T, at + a, run_at + a, dc2, R, max_d2, best);
        }
        const bool found = best != Z_NONE;
        const int32_t d2 = found ? (int32_t)(best >> 16) : 0, other = found ? (int32_t)(best & 0xffffu) : 0;
        const int32_t depth = found ? d2 : SDSM_ZONE_NO_UPPER;       // d2 with "nothing found" as +infinity
        const int64_t px = S.off[im] + (int64_t)r * W + c;
        if (d2_out_) d2_out_[px] = d2;
        if (other_out_) other_out_[px] = other;
        for (int z = 0; z < S.n_zones; z++) {
            const sdsm_zone_spec &Z = S.zone[z];
            const bool in = depth > Z.lo_d2 && depth <= Z.hi_d2;
            int32_t v = 0;
            if (l != 0) { if (Z.keep_own || (Z.side == SDSM_ZONE_SIDE_OBJECT && in)) v = (int32_t)l; }
            else if (Z.side == SDSM_ZONE_SIDE_BACKGROUND && in) v = other;
            zone_out_[z * stride + px] = v;
        }
    }
}

template <int HALO> void launch(const ZSet &S, const int32_t *labels, int32_t *d2, int32_t *other, int32_t *zone_out, int32_t *status, hipStream_t stream)
{
    hipLaunchKernelGGL(k_zones<HALO>, dim3(S.start[S.n]), dim3(ZTPB), 0, stream, S, labels, d2, other, zone_out, status);
}

}  // namespace

// The status words are cleared here, on the stream; every pixel of every map asked for is written by the kernel.
extern "C" hipError_t sdsm_zones_impl(const sdsm_set_image *images, int n_images, const int32_t *d_labels, int max_d2, int n_zones,
                                      const sdsm_zone_spec *zones, int64_t zone_stride, int32_t *d_d2, int32_t *d_other, int32_t *d_zone_out,
                                      int32_t *d_status, hipStream_t stream)
{
    ZSet S{};
    S.n = n_images;
    S.max_d2 = max_d2;
    S.reach = sdsm_neighbour_isqrt_inline(max_d2);
    S.n_zones = n_zones;
    S.zone_stride = zone_stride;
    for (int z = 0; z < n_zones; z++) S.zone[z] = zones[z];
    for (int i = 0; i < n_images; i++) {
        S.H[i] = images[i].H; S.W[i] = images[i].W; S.off[i] = images[i].offset;
        S.tiles_w[i] = (images[i].W + ZTW - 1) / ZTW;
        S.start[i + 1] = S.start[i] + S.tiles_w[i] * ((images[i].H + ZTH - 1) / ZTH);
    }
    hipError_t e = hipMemsetAsync(d_status, 0, (size_t)n_images * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (S.reach <= 4) launch<4>(S, d_labels, d_d2, d_other, d_zone_out, d_status, stream);
    else if (S.reach <= 16) launch<16>(S, d_labels, d_d2, d_other, d_zone_out, d_status, stream);
    else launch<64>(S, d_labels, d_d2, d_other, d_zone_out, d_status, stream);
    return hipGetLastError();
}
