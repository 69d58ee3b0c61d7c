// Skeleton tables on the GPU: one sdsm_skeleton_record and the skeleton's bits per object (bit-packed fragments) or per label (the windows
// of sdsm_shape.hip), for one image or a set of images.  No reference counterpart; the definition the kernel is tested against is the
// host code of superdsm_amd/skeleton.py, and the word functions are those of sdsm_skeleton.h, which the host helpers compile too.
//
//   k_skeleton   one workgroup of 256 threads per four objects.  The whole thinning of an object happens inside the launch: no global
//                flag, no waiting between workgroups, no atomics, no output that needs clearing (but the label map, which the entry
//                clears in stream order first).
//     wavefront path   h <= 64 and w <= 64: wavefront q of the workgroup takes object 4 b + q.  Lane r holds row r as one 64-bit word in
//                      a register; the rows above and below come by lane shuffles, east, west and the diagonals by shifts; "anything
//                      removed" is a wavefront vote.  No LDS traffic and no barrier in the loop.
//     LDS path         h * ceil(w / 64) <= SDSM_SKELETON_LDS_WORDS: after the wavefront objects, the whole workgroup takes each remaining
//                      object of its four in turn.  Two planes of row-aligned words in LDS; a subiteration reads the nine words around
//                      each word of one plane (a word outside the box reads 0, so bits cross the word seams by the shifts of
//                      sdsm_skeleton_planes) and writes the other plane; then a barrier.  Termination is a workgroup OR after the four
//                      subiterations of a cycle.
//     workspace path   larger boxes: the same code over two planes in the caller's workspace: the same bytes, more slowly.
//   Every path unpacks the flat window bits into row-aligned words, writes the skeleton back in the flat layout (and the label at the
//   skeleton's pixels of the label map) and reduces the record in integers.  The path is chosen by the box alone.
#include "sdsm_tables.h"
#include "sdsm_skeleton.h"
#include <climits>

static_assert(SDSM_SKELETON_LDS_WORDS == SDSM_SKELETON_LDS_WORDS_INLINE, "the limit of include/sdsm.h and of the inline header");
static_assert(sizeof(sdsm_skeleton_record) == 48, "the size of include/sdsm.h and of _capi.py");

namespace {

constexpr int STPB = 256;                        // threads of a workgroup
constexpr int SWAVES = STPB / 64;                // = objects of a workgroup
constexpr int LW = SDSM_SKELETON_LDS_WORDS;
static_assert(LW >= SWAVES * 64, "the wavefront path stages its 64 rows per wavefront in the first plane");

struct SLds {                                    // 48.3 KB: three workgroups per compute unit
    u64 plane[2][LW];
    int32_t red[SWAVES][12];
    int32_t any[SWAVES];
};

struct Partial {                                 // what a thread has seen of its object
    int32_t area, cmin, cmax, rmin, rmax;        // of P: its pixels and its tight box, in box coordinates
};

__device__ __forceinline__ void see(Partial &P, u64 word, int r, int j)
{
    if (!word) return;
    P.area += __builtin_popcountll(word);
    const int lo = 64 * j + __builtin_ctzll(word), hi = 64 * j + 63 - __builtin_clzll(word);
    P.cmin = lo < P.cmin ? lo : P.cmin; P.cmax = hi > P.cmax ? hi : P.cmax;
    P.rmin = r < P.rmin ? r : P.rmin; P.rmax = r > P.rmax ? r : P.rmax;
}

__device__ __forceinline__ void write_record(sdsm_skeleton_record *out, const int32_t *v, int cycles, const Fragment &f)
{
    // v: area, n_skeleton, n_end, n_isolated, n_branch, n_orth, n_diag, first (flat index in the box), cmin, rmin, -cmax, -rmax
    sdsm_skeleton_record R;
    R.area = v[0]; R.n_skeleton = v[1]; R.n_end = v[2]; R.n_isolated = v[3]; R.n_branch = v[4]; R.n_orth = v[5]; R.n_diag = v[6];
    R.cycles = cycles;
    R.first_row = R.first_col = 0; R.flags = 0; R.reserved = 0;
    if (v[0] > 0) {
        R.first_row = f.r0 + v[7] / f.w; R.first_col = f.c0 + v[7] % f.w;
        R.flags = (f.r0 + v[9] == 0 || f.c0 + v[8] == 0 || f.r0 - v[11] + 1 == f.H || f.c0 - v[10] + 1 == f.W) ? 1 : 0;
    }
    *out = R;
}

__device__ __forceinline__ void zero_record(sdsm_skeleton_record *out, int flags)
{
    sdsm_skeleton_record R;
    R.area = R.n_skeleton = R.n_end = R.n_isolated = R.n_branch = R.n_orth = R.n_diag = R.cycles = R.first_row = R.first_col = R.reserved = 0;
    R.flags = flags;
    *out = R;
}

// the nine words around word (r, j) of a plane of h rows of nw words
__device__ __forceinline__ u64 around(const u64 *A, int h, int nw, int r, int j, u64 n[8])
{
    u64 up[3], row[3], down[3];
    const u64 *p = A + (int64_t)r * nw + j;
    const bool l = j > 0, rt = j + 1 < nw, u = r > 0, d = r + 1 < h;
    row[0] = l ? p[-1] : 0; row[1] = p[0]; row[2] = rt ? p[1] : 0;
    up[0] = u && l ? p[-nw - 1] : 0; up[1] = u ? p[-nw] : 0; up[2] = u && rt ? p[-nw + 1] : 0;
    down[0] = d && l ? p[nw - 1] : 0; down[1] = d ? p[nw] : 0; down[2] = d && rt ? p[nw + 1] : 0;
    sdsm_skeleton_planes(up, row, down, n);
    return row[1];
}

// One subiteration of direction D over the plane A into the plane B by the STPB threads of the workgroup; != 0 where this thread removed
template <int D>
__device__ __forceinline__ int subiteration(const u64 *A, u64 *B, int h, int nw, int tid)
{
    int removed = 0;
    const int total = h * nw;
    int r = tid / nw, j = tid % nw;
    const int dr = STPB / nw, dj = STPB % nw;
    for (int idx = tid; idx < total; idx += STPB) {
        u64 c = A[idx];
        if (c) {                                 // (an empty word stays empty and costs one read)
            u64 n[8];
            around(A, h, nw, r, j, n);
            const u64 rm = sdsm_skeleton_remove(c, n, D);
            c &= ~rm;
            removed |= rm != 0;
        }
        B[idx] = c;
        r += dr; j += dj;
        if (j >= nw) { j -= nw; r++; }
    }
    return removed;
}

// The record of the skeleton in the plane A (complete and visible to the T threads that call this: a wavefront, T = 64, or the workgroup,
// T = 256), its flat bits and its pixels of the label map.  t: the thread among the T.
template <int T>
__device__ __forceinline__ void finish(SLds &L, const u64 *A, const Fragment &f, int nw, int t, Partial P, int cycles, sdsm_skeleton_record *out,
                                       uint32_t *skel, int32_t label, int32_t *map)
{
    const int h = f.h, total = h * nw;
    sdsm_skeleton_counts K = {0, 0, 0, 0, 0, 0};
    int32_t first = INT_MAX;
    int r = t / nw, j = t % nw;
    const int dr = T / nw, dj = T % nw;
    for (int idx = t; idx < total; idx += T) {
        u64 n[8];
        u64 c = around(A, h, nw, r, j, n);
        if (c) {
            sdsm_skeleton_classify(c, n, K);
            const int32_t p = r * f.w + 64 * j + __builtin_ctzll(c);             // (< h w < 2^31)
            first = p < first ? p : first;
            if (map) {
                int32_t *row = map + (int64_t)(f.r0 + r) * f.W + f.c0 + 64 * j;
                while (c) {
                    row[__builtin_ctzll(c)] = label;
                    c &= c - 1;
                }
            }
        }
        r += dr; j += dj;
        if (j >= nw) { j -= nw; r++; }
    }
    const uint32_t n_bits = (uint32_t)h * (uint32_t)f.w, n32 = (n_bits + 31) >> 5;
    for (uint32_t k = t; k < n32; k += T) skel[k] = sdsm_skeleton_flat_word(A, (uint32_t)f.w, (uint32_t)nw, n_bits, k);

    int32_t v[12] = {P.area, K.n_skeleton, K.n_end, K.n_isolated, K.n_branch, K.n_orth, K.n_diag, first, P.cmin, P.rmin, -P.cmax, -P.rmax};
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const int32_t x = __shfl_down(v[i], o);
            v[i] = i < 7 ? v[i] + x : (x < v[i] ? x : v[i]);
        }
    }
    if (T == 64) {
        if (t == 0) write_record(out, v, cycles, f);
        return;
    }
    __syncthreads();                             // (red may still be read for the object before)
    if ((t & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 12; i++) L.red[t >> 6][i] = v[i];
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < SWAVES; k++) {
#pragma unroll
            for (int i = 0; i < 12; i++) {
                const int32_t x = L.red[k][i];
                v[i] = i < 7 ? v[i] + x : (x < v[i] ? x : v[i]);
            }
        }
        write_record(out, v, cycles, f);
    }
}

// The object in a box of at most 64 x 64 by one wavefront
__device__ __forceinline__ void skeleton_wave(SLds &L, const Fragment &f, const uint32_t *bits, int lane, int wave, sdsm_skeleton_record *out, uint32_t *skel,
                                              int32_t label, int32_t *map)
{
    const uint32_t n_bits = (uint32_t)f.h * (uint32_t)f.w, n32 = (n_bits + 31) >> 5;
    u64 x = lane < f.h ? sdsm_skeleton_flat_bits(bits, n32, (uint32_t)lane * (uint32_t)f.w, f.w) : 0;
    Partial P = {0, INT_MAX, -1, INT_MAX, -1};
    see(P, x, lane, 0);
    int cycles = 0;
    for (;;) {
        int removed = 0;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const u64 a = __shfl_up(x, 1), b = __shfl_down(x, 1);
            const u64 up[3] = {0, lane > 0 ? a : 0, 0}, row[3] = {0, x, 0}, down[3] = {0, lane < 63 ? b : 0, 0};
            u64 n[8];
            sdsm_skeleton_planes(up, row, down, n);
            const u64 rm = s == 0 ? sdsm_skeleton_remove(x, n, 0) : s == 1 ? sdsm_skeleton_remove(x, n, 4) : s == 2 ? sdsm_skeleton_remove(x, n, 2)
                                                                                                                     : sdsm_skeleton_remove(x, n, 6);
            x &= ~rm;
            removed |= rm != 0;
        }
        if (!__any(removed)) break;
        cycles++;
    }
    u64 *A = L.plane[0] + 64 * wave;             // the rows staged for the classifiers and the flat bits: this wavefront's own 64 words
    A[lane] = x;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    finish<64>(L, A, f, 1, lane, P, cycles, out, skel, label, map);
}

// The object in a larger box by the workgroup, over the planes A and B (LDS or workspace)
__device__ __forceinline__ void skeleton_block(SLds &L, u64 *A, u64 *B, const Fragment &f, const uint32_t *bits, int tid, sdsm_skeleton_record *out,
                                               uint32_t *skel, int32_t label, int32_t *map)
{
    const int h = f.h, nw = (f.w + 63) >> 6, total = h * nw;
    const uint32_t n_bits = (uint32_t)h * (uint32_t)f.w, n32 = (n_bits + 31) >> 5;
    Partial P = {0, INT_MAX, -1, INT_MAX, -1};
    for (int idx = tid; idx < total; idx += STPB) {
        const int r = idx / nw, j = idx % nw;
        const int cnt = f.w - 64 * j < 64 ? f.w - 64 * j : 64;
        const u64 word = sdsm_skeleton_flat_bits(bits, n32, (uint32_t)r * (uint32_t)f.w + 64u * (uint32_t)j, cnt);
        A[idx] = word;
        see(P, word, r, j);
    }
    __syncthreads();
    int cycles = 0;
    for (;;) {
        int removed = subiteration<0>(A, B, h, nw, tid);
        __syncthreads();
        removed |= subiteration<4>(B, A, h, nw, tid);
        __syncthreads();
        removed |= subiteration<2>(A, B, h, nw, tid);
        __syncthreads();
        removed |= subiteration<6>(B, A, h, nw, tid);
        const int any = __any(removed);
        if ((tid & 63) == 0) L.any[tid >> 6] = any;
        __syncthreads();                         // (any is written again three barriers on at the earliest)
        if (!(L.any[0] | L.any[1] | L.any[2] | L.any[3])) break;
        cycles++;
    }
    finish<STPB>(L, A, f, nw, tid, P, cycles, out, skel, label, map);
}

__global__ __launch_bounds__(STPB) void k_skeleton(SetImages S, int n, const int32_t *obj_image, const int32_t *boxes, const int64_t *bits_off,
                                                   const uint32_t *bits_, const int64_t *ws_off, u64 *ws, int64_t ws_words, sdsm_skeleton_record *out,
                                                   uint32_t *skel_, const int32_t *obj_label, int32_t *map_)
{
    __shared__ SLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {                                            // ---- the wavefront objects: no barrier in here --------------------------------------------
        const int i = SWAVES * blockIdx.x + wave;
        if (i < n) {                             // (uniform in the wavefront, as everything below that depends on i alone)
            const int im = obj_image ? obj_image[i] : 0;
            Fragment f;
            if (!fragment_box(S, im, boxes, i, f)) {
                if (lane == 0) zero_record(out + i, 0);
            } else if (f.h <= 64 && f.w <= 64) {
                skeleton_wave(L, f, bits_ + bits_off[i], lane, wave, out + i, skel_ + bits_off[i], obj_label ? obj_label[i] : 0, map_ ? map_ + S.off[im] : nullptr);
            }
        }
    }
    __syncthreads();
    for (int q = 0; q < SWAVES; q++) {           // ---- the larger objects, one after the other by the whole workgroup -------------------------
        const int i = SWAVES * blockIdx.x + q;
        if (i >= n) break;                       // (uniform in the workgroup)
        const int im = obj_image ? obj_image[i] : 0;
        Fragment f;
        if (!fragment_box(S, im, boxes, i, f) || (f.h <= 64 && f.w <= 64)) continue;
        const int64_t words = (int64_t)f.h * ((f.w + 63) >> 6);
        u64 *A = L.plane[0], *B = L.plane[1];
        if (words > LW) {
            const int64_t off = ws_off ? ws_off[i] : -1;
            if (!ws || off < 0 || off > ws_words - 2 * words) {                   // no room named for this box: flagged, nothing is written there
                if (tid == 0) zero_record(out + i, SDSM_SKELETON_NO_WORKSPACE);
                continue;
            }
            A = ws + off; B = A + words;
        }
        __syncthreads();                         // (the planes may still be read for the object before)
        skeleton_block(L, A, B, f, bits_ + bits_off[i], tid, out + i, skel_ + bits_off[i], obj_label ? obj_label[i] : 0, map_ ? map_ + S.off[im] : nullptr);
    }
}

}  // namespace

extern "C" hipError_t sdsm_skeleton_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                 const int64_t *bits_off, const uint32_t *bits, const int64_t *d_ws_off, void *d_ws, int64_t ws_words,
                                                 sdsm_skeleton_record *out, uint32_t *skel, const int32_t *obj_label, int32_t *map, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const SetImages S = make_set(images, n_images);
    hipLaunchKernelGGL(k_skeleton, dim3((n + SWAVES - 1) / SWAVES), dim3(STPB), 0, stream, S, n, obj_image, boxes, bits_off, bits, d_ws_off, (u64 *)d_ws, ws_words, out,
                       skel, obj_label, map);
    return hipGetLastError();
}
