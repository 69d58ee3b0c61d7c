// Per-object work of the post-processing stage, one workgroup per object, one launch per set of images
// (sdsm_k_post_set: the image of an object comes from the launch's table; a single image is the set of one).
//
// Reference behaviour restated here (never its code):
//   contrast response           superdsm/postprocess.py:254-266  (_compute_contrast)
//   mask refinement             superdsm/postprocess.py:316-337  (_process_mask; its hole filling: sdsm_k_post_fill below)
// The reference evaluates both on FULL-IMAGE arrays per object (a Euclidean distance transform of the whole image for every
// object).  Neither needs more than a window around the object: the exterior weights vanish beyond exterior_offset + 5 *
// exterior_scale pixels from the mask, the refinement only touches pixels within mask_max_distance of its boundary.
//   exterior distance of a pixel = sqrt of the smallest integer squared distance to a mask pixel -- what
//   scipy.ndimage.distance_transform_edt returns; the nearest mask pixel of an outside pixel is a boundary pixel of the mask, so
//   the minimum runs over the boundary list (LDS) only.
#include "sdsm_common.h"
#include "sdsm_set.h"

namespace {

#define POST_WG 256
#define POST_MAX_BOUNDARY 12288          // boundary pixels kept in LDS (48 KB); larger objects use the global list

struct PostParams {
    int32_t H, W, n;
    int32_t max_distance;                // postprocess/mask_max_distance (disk radius), 0: no refinement
    double exterior_scale, exterior_offset, contrast_epsilon, inv_gstd;   // inv_gstd = 1 / g.std() (postprocess.py:255)
    double stdamp;
    const double *g, *gs;                // raw intensities; Gaussian-smoothed intensities of the refinement (postprocess.py:165)
    const uint8_t *bg;                   // background_mask (postprocess.py:152-155)
    const int32_t *boxes;                // n x 4: r0, c0, h, w of the fragments
    const int64_t *bits_off;             // first uint32 word of each fragment's bits (row-major, LSB first)
    const uint32_t *bits;
    const int64_t *new_off;              // first word of each refined mask (window = box +- max_distance, clamped to the image)
    uint32_t *new_bits;
    uint32_t *boundary_pool;             // global boundary lists for objects beyond POST_MAX_BOUNDARY: bpool_off[i] .. (may be null)
    const int64_t *bpool_off;
    sdsm_post_record *out;
};

__device__ __forceinline__ bool frag_bit(const uint32_t *bits, int h, int w, int r, int c)
{
    if (r < 0 || c < 0 || r >= h || c >= w) return false;
    const int b = r * w + c;
    return (bits[b >> 5] >> (b & 31)) & 1u;
}

}  // namespace

// object i of P (one workgroup): the body of sdsm_k_post_set
__device__ __forceinline__ void post_object(const PostParams &P, int i)
{
    __shared__ uint32_t bnd[POST_MAX_BOUNDARY];
    __shared__ double red[POST_WG / 64 * 8];
    __shared__ int nb_sh, ired[POST_WG / 64];
    const int tid = threadIdx.x;
    const int r0 = P.boxes[4 * i], c0 = P.boxes[4 * i + 1], h = P.boxes[4 * i + 2], w = P.boxes[4 * i + 3];
    const uint32_t *bits = P.bits + P.bits_off[i];
    if (tid == 0) nb_sh = 0;
    __syncthreads();

    // ---- A. interior statistics and the boundary list ------------------------------------------------------------------------
    double s_g = 0, s_gs = 0;
    int cnt = 0;
    uint32_t *blist = bnd;
    const bool use_pool = P.boundary_pool != nullptr && P.bpool_off[i] >= 0;
    if (use_pool) blist = P.boundary_pool + P.bpool_off[i];
    for (int e = tid; e < h * w; e += POST_WG) {
        const int r = e / w, c = e - r * w;
        if (!frag_bit(bits, h, w, r, c)) continue;
        const size_t p = (size_t)(r0 + r) * P.W + (c0 + c);
        const double gv = P.g[p], sv = P.gs[p];
        s_g += gv; s_gs += sv; cnt++;
        if (!(frag_bit(bits, h, w, r - 1, c) && frag_bit(bits, h, w, r + 1, c) && frag_bit(bits, h, w, r, c - 1) && frag_bit(bits, h, w, r, c + 1))) {
            const int k = atomicAdd(&nb_sh, 1);
            if (use_pool || k < POST_MAX_BOUNDARY) blist[k] = ((uint32_t)(r0 + r) << 16) | (uint32_t)(c0 + c);
        }
    }
    double v3[3] = {s_g, s_gs, (double)cnt};
#pragma unroll
    for (int k = 0; k < 3; k++) v3[k] = wave_sum(v3[k]);
    __syncthreads();
    if ((tid & 63) == 0) for (int k = 0; k < 3; k++) red[(tid >> 6) * 8 + k] = v3[k];
    __syncthreads();
    double tot[3] = {0, 0, 0};
    for (int wv = 0; wv < POST_WG / 64; wv++) for (int k = 0; k < 3; k++) tot[k] += red[wv * 8 + k];
    const int nb = nb_sh;
    const double area = tot[2];
    sdsm_post_record rec = {};
    rec.area = (int32_t)area;
    if (!use_pool && nb > POST_MAX_BOUNDARY) {           // the host did not reserve a global list for this object
        if (tid == 0) { rec.status = 1; P.out[i] = rec; }
        return;
    }
    if (area == 0) { if (tid == 0) { rec.status = 2; P.out[i] = rec; } return; }
    const double interior_mean = (tot[0] / area) * P.inv_gstd;
    const double fg_mean = tot[1] / area;
    // population variance (numpy std) in a second pass over the fragment, with the mean known: sum(sv^2) / area - mean^2 loses
    // every digit of the deviation that lies below eps * mean^2 (an image with a large constant level)
    double s_d2 = 0;
    for (int e = tid; e < h * w; e += POST_WG) {
        const int r = e / w, c = e - r * w;
        if (!frag_bit(bits, h, w, r, c)) continue;
        const double d = P.gs[(size_t)(r0 + r) * P.W + (c0 + c)] - fg_mean;
        s_d2 += d * d;
    }
    s_d2 = wave_sum(s_d2);
    __syncthreads();
    if ((tid & 63) == 0) red[(tid >> 6) * 8] = s_d2;
    __syncthreads();
    double var = 0;
    for (int wv = 0; wv < POST_WG / 64; wv++) var += red[wv * 8];
    var /= area;
    const double fg_amp = sqrt(var) * P.stdamp;
    __syncthreads();

    // ---- B. exterior mean (postprocess.py:260-265): weights exp(-max(0, d - offset) / scale) where that exponent is <= 5 ------
    const double reach = P.exterior_offset + 5.0 * P.exterior_scale;
    const int D = (int)ceil(reach);
    const int wr0 = r0 - D < 0 ? 0 : r0 - D, wc0 = c0 - D < 0 ? 0 : c0 - D;
    const int wr1 = r0 + h + D > P.H ? P.H : r0 + h + D, wc1 = c0 + w + D > P.W ? P.W : c0 + w + D;
    const int ww = wc1 - wc0, wh = wr1 - wr0;
    double s_w = 0, s_gw = 0;
    for (int e = tid; e < wh * ww; e += POST_WG) {
        const int r = wr0 + e / ww, c = wc0 + e % ww;
        if (frag_bit(bits, h, w, r - r0, c - c0)) continue;              // xor with the mask: mask pixels have distance 0 <= 5
        const size_t p = (size_t)r * P.W + c;
        if (!P.bg[p]) continue;
        long long best = 1ll << 60;
        for (int k = 0; k < nb; k++) {
            const uint32_t q = blist[k];
            const long long dr = (long long)(q >> 16) - r, dc = (long long)(q & 0xffffu) - c;
            const long long d2 = dr * dr + dc * dc;
            best = d2 < best ? d2 : best;
        }
        double t = sqrt((double)best) - P.exterior_offset;
        t = (t < 0 ? 0 : t) / P.exterior_scale;
        if (t <= 5.0) {
            const double wgt = exp(-t);
            s_w += wgt; s_gw += wgt * (P.g[p] * P.inv_gstd);
        }
    }
    double v2[2] = {s_w, s_gw};
#pragma unroll
    for (int k = 0; k < 2; k++) v2[k] = wave_sum(v2[k]);
    __syncthreads();
    if ((tid & 63) == 0) for (int k = 0; k < 2; k++) red[(tid >> 6) * 8 + k] = v2[k];
    __syncthreads();
    double sw = 0, sgw = 0;
    for (int wv = 0; wv < POST_WG / 64; wv++) { sw += red[wv * 8]; sgw += red[wv * 8 + 1]; }
    const double exterior_mean = sgw / sw;               // 0 / 0 = NaN when nothing qualifies, as the reference's division does
    rec.interior_mean = interior_mean; rec.exterior_mean = exterior_mean;
    rec.contrast = (interior_mean + P.contrast_epsilon) / (exterior_mean + P.contrast_epsilon);
    rec.fg_mean = fg_mean; rec.fg_std = sqrt(var);

    // ---- C. mask refinement (postprocess.py:316-337): pixels within disk(max_distance) of the mask boundary join the mask iff
    //      their smoothed intensity lies within stdamp standard deviations of the mask's mean ------------------------------------
    const int m = P.max_distance;
    int rmin = 1 << 30, rmax = -1, cmin = 1 << 30, cmax = -1;
    if (m > 0 && P.stdamp > 0) {
        const int nr0 = r0 - m < 0 ? 0 : r0 - m, nc0 = c0 - m < 0 ? 0 : c0 - m;
        const int nr1 = r0 + h + m > P.H ? P.H : r0 + h + m, nc1 = c0 + w + m > P.W ? P.W : c0 + w + m;
        const int nw = nc1 - nc0, nh = nr1 - nr0;
        uint32_t *nbits = P.new_bits + P.new_off[i];
        __syncthreads();
        for (int e = tid; e < (nh * nw + 31) / 32; e += POST_WG) nbits[e] = 0;
        __syncthreads();
        for (int e = tid; e < nh * nw; e += POST_WG) {
            const int r = nr0 + e / nw, c = nc0 + e % nw;
            const bool in = frag_bit(bits, h, w, r - r0, c - c0);
            bool any = false, all = true;                                 // dilation / erosion by the disk footprint
            for (int dr = -m; dr <= m; dr++) for (int dc = -m; dc <= m; dc++) {
                if (dr * dr + dc * dc > m * m) continue;
                const int rr = r + dr, cc = c + dc;
                const bool inside_image = rr >= 0 && cc >= 0 && rr < P.H && cc < P.W;
                const bool b = inside_image ? frag_bit(bits, h, w, rr - r0, cc - c0) : false;
                any |= b;
                all &= inside_image ? b : true;                            // erosion: outside the image counts as foreground
            }
            bool v = in;
            if (any != all) {                                              // dilation xor erosion (erosion implies dilation)
                const double sv = P.gs[(size_t)r * P.W + c];
                v = fg_mean - fg_amp <= sv && sv <= fg_mean + fg_amp;
            }
            if (v) {
                atomicOr(&nbits[e >> 5], 1u << (e & 31));
                rmin = r < rmin ? r : rmin; rmax = r > rmax ? r : rmax; cmin = c < cmin ? c : cmin; cmax = c > cmax ? c : cmax;
            }
        }
        rmin = block_min_i32<POST_WG / 64>(rmin, ired); cmin = block_min_i32<POST_WG / 64>(cmin, ired);
        rmax = -block_min_i32<POST_WG / 64>(-rmax, ired); cmax = -block_min_i32<POST_WG / 64>(-cmax, ired);
        if (rmax >= 0) { rec.r0 = rmin; rec.c0 = cmin; rec.h = rmax - rmin + 1; rec.w = cmax - cmin + 1; }
    } else { rec.r0 = r0; rec.c0 = c0; rec.h = h; rec.w = w; rec.status = 3; }   // no refinement on the device
    if (tid == 0) P.out[i] = rec;
}

namespace {

// the objects of a set of images: the shared parameters and per-object arrays in P, the per-image inputs in the table
struct PostSetParams {
    PostParams P;
    int32_t n_images;
    int32_t first[SDSM_MAX_SET_IMAGES + 1];      // prefix of the images' object counts
    sdsm_post_image im[SDSM_MAX_SET_IMAGES];
};

}  // namespace

__global__ __launch_bounds__(POST_WG) void sdsm_k_post_set(PostSetParams S)
{
    const sdsm_post_image &im = S.im[set_find(S.first, S.n_images, blockIdx.x)];
    PostParams P = S.P;
    P.H = im.H; P.W = im.W; P.n = im.n_objects; P.inv_gstd = im.inv_gstd;
    P.g = im.d_g; P.gs = im.d_gs; P.bg = im.d_bg;
    post_object(P, blockIdx.x);
}

extern "C" hipError_t sdsm_launch_post_set(const sdsm_post_image *images, int n_images, const int32_t *boxes, const int64_t *bits_off,
                                           const uint32_t *bits, const int64_t *new_off, uint32_t *new_bits, uint32_t *boundary_pool,
                                           const int64_t *bpool_off, double exterior_scale, double exterior_offset, double contrast_epsilon,
                                           int max_distance, double stdamp, sdsm_post_record *out, hipStream_t stream)
{
    PostSetParams S{};
    S.n_images = n_images;
    S.first[0] = 0;
    for (int j = 0; j < n_images; j++) {
        S.im[j] = images[j];
        S.first[j + 1] = S.first[j] + images[j].n_objects;
    }
    const int n = S.first[n_images];
    if (n <= 0) return hipSuccess;
    PostParams &P = S.P;
    P.max_distance = max_distance;
    P.exterior_scale = exterior_scale; P.exterior_offset = exterior_offset; P.contrast_epsilon = contrast_epsilon; P.stdamp = stdamp;
    P.boxes = boxes; P.bits_off = bits_off; P.bits = bits; P.new_off = new_off; P.new_bits = new_bits;
    P.boundary_pool = boundary_pool; P.bpool_off = bpool_off; P.out = out;
    hipLaunchKernelGGL(sdsm_k_post_set, dim3(n), dim3(POST_WG), 0, stream, S);
    return hipGetLastError();
}

// =====================================================================================================================================
// The exact bit problems of the stage: hole filling, the glare test, the background mask.
//
// Hole filling and the glare test share one primitive, a bit-parallel constrained flood over a window: `reached |= (reached moved
// up / down / left / right) & allowed` until nothing changes.  The project's fragment format is row-major with CONTINUOUS bits (a row
// starts wherever the one before ended), so a window is first re-packed to whole words per row (wpr = ceil(w / 32) words, the bits
// past w clear); up / down are then the same word of the neighbouring row, left / right a shift with the neighbouring word's end bit.
// Within a word the flood does not walk: adding the seeds to the allowed bits lets the carry run through every run of allowed bits
// above a seed ((allowed + seeds) ^ allowed), the bit-reversed words give the runs below.  A thread owns one word column of a band of
// rows and sweeps it down and up, so a pass moves the front a whole band vertically and a whole word horizontally.  Words are only
// ever OR-ed into by their owner, so a stale read of a neighbour costs a pass, never a bit.  4-connectivity throughout: what
// scipy.ndimage.binary_fill_holes and scipy.ndimage.label use by default.
//
// A window of at most POST_FLOOD_WORDS words per plane is flooded in LDS; a larger one in the caller's global workspace by the same
// workgroup (correct, slow).
// =====================================================================================================================================
namespace {

#define POST_FLOOD_WORDS 4096            // words of one bit plane in LDS (16 KB): h * ceil(w / 32) beyond it floods in global memory
#define POST_FLOOD_BAND 8                // rows a thread sweeps per pass

__device__ __forceinline__ uint32_t row_mask(int w, int j)          // the bits of word j of a row of w pixels
{
    const int n = w - 32 * j;
    return n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
}

// word j of row r of an h x w fragment in the continuous format (n_words words)
__device__ __forceinline__ uint32_t load_row_word(const uint32_t *bits, int64_t n_words, int w, int r, int j)
{
    const int64_t start = (int64_t)r * w + 32 * j, k = start >> 5;
    const int sh = (int)(start & 31);
    uint32_t v = bits[k] >> sh;
    if (sh && k + 1 < n_words) v |= bits[k + 1] << (32 - sh);
    return v & row_mask(w, j);
}

// word k of the continuous format from the row-packed plane
__device__ __forceinline__ uint32_t gather_word(const uint32_t *plane, int h, int w, int wpr, int64_t k)
{
    int64_t p = 32 * k;
    const int64_t total = (int64_t)h * w, end = p + 32 < total ? p + 32 : total;
    uint32_t out = 0;
    while (p < end) {
        const int r = (int)(p / w), c = (int)(p - (int64_t)r * w), s = c & 31;
        int n = 32 - s;
        n = w - c < n ? w - c : n;
        n = end - p < n ? (int)(end - p) : n;
        uint32_t v = plane[(size_t)r * wpr + (c >> 5)] >> s;
        if (n < 32) v &= (1u << n) - 1u;
        out |= v << (int)(p - 32 * k);
        p += n;
    }
    return out;
}

// the runs of `a` that hold a bit of x (x within a), upwards and downwards
__device__ __forceinline__ uint32_t smear(uint32_t x, uint32_t a)
{
    x |= ((a + x) ^ a) & a;
    const uint32_t ra = __brev(a), rx = __brev(x);
    return x | __brev(((ra + rx) ^ ra) & ra);
}

// a * b + c in two rounded operations, as NumPy evaluates the glare threshold: hipcc contracts the expression to one fused
// multiply-add by default (and __dmul_rn / __dadd_rn are plain operators in its headers, contracted alike), which would move ties
__device__ __forceinline__ double mul_then_add(double a, double b, double c)
{
#pragma clang fp contract(off)
    const double p = a * b;
    return p + c;
}

// reached (within allowed) grows to the 4-connected components of allowed it touches; all threads of the workgroup call it
__device__ __forceinline__ void flood(const uint32_t *allowed, uint32_t *reached, int h, int wpr, int *changed)
{
    const int tid = threadIdx.x;
    const int bands = (h + POST_FLOOD_BAND - 1) / POST_FLOOD_BAND;
    const int64_t items = (int64_t)bands * wpr;
    auto relax = [&](int r, int j) -> bool {
        const size_t idx = (size_t)r * wpr + j;
        const uint32_t a = allowed[idx];
        if (!a) return false;
        const uint32_t old = reached[idx];
        uint32_t x = old | (old << 1) | (old >> 1);
        if (r > 0) x |= reached[idx - wpr];
        if (r + 1 < h) x |= reached[idx + wpr];
        if (j > 0) x |= reached[idx - 1] >> 31;
        if (j + 1 < wpr) x |= reached[idx + 1] << 31;
        x = smear(x & a, a);
        if (x == old) return false;
        reached[idx] = x;
        return true;
    };
    for (;;) {
        __syncthreads();
        if (tid == 0) *changed = 0;
        __syncthreads();
        bool ch = false;
        for (int64_t it = tid; it < items; it += POST_WG) {
            const int j = (int)(it % wpr), lo = (int)(it / wpr) * POST_FLOOD_BAND;
            const int hi = lo + POST_FLOOD_BAND < h ? lo + POST_FLOOD_BAND : h;
            for (int r = lo; r < hi; r++) ch |= relax(r, j);
            for (int r = hi - 2; r >= lo; r--) ch |= relax(r, j);
        }
        if (ch) *changed = 1;
        __syncthreads();
        if (!*changed) break;
    }
}

struct FillParams {
    int32_t n;
    const int32_t *dims;                 // n x 2: h, w
    const int64_t *off;                  // first word of each window, in and out
    const uint32_t *in;
    uint32_t *out;
    uint32_t *ws;                        // two planes for every window beyond POST_FLOOD_WORDS at ws + ws_off[i] (may be null)
    const int64_t *ws_off;
    int32_t *status;                     // 0 filled, 1 the window needs a workspace and has none
};

}  // namespace

// scipy.ndimage.binary_fill_holes (default structure) of window blockIdx.x: the background is flooded from the window's border, what
// the flood does not reach is filled
__global__ __launch_bounds__(POST_WG) void sdsm_k_post_fill(FillParams F)
{
    __shared__ uint32_t planes[2 * POST_FLOOD_WORDS];
    __shared__ int changed;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int h = F.dims[2 * i], w = F.dims[2 * i + 1], wpr = (w + 31) >> 5;
    const int64_t words = (int64_t)h * wpr, n_words = ((int64_t)h * w + 31) >> 5;
    const uint32_t *src = F.in + F.off[i];
    uint32_t *dst = F.out + F.off[i];
    uint32_t *allowed = planes, *reached = planes + POST_FLOOD_WORDS;
    if (words > POST_FLOOD_WORDS) {
        if (!F.ws || !F.ws_off || F.ws_off[i] < 0) { if (tid == 0) F.status[i] = 1; return; }
        allowed = F.ws + F.ws_off[i];
        reached = allowed + words;
    }
    for (int64_t e = tid; e < words; e += POST_WG) {
        const int r = (int)(e / wpr), j = (int)(e - (int64_t)r * wpr);
        const uint32_t rm = row_mask(w, j), a = ~load_row_word(src, n_words, w, r, j) & rm;
        uint32_t border = (r == 0 || r == h - 1) ? rm : 0u;
        if (j == 0) border |= 1u;
        if (j == wpr - 1) border |= 1u << ((w - 1) & 31);
        allowed[e] = a;
        reached[e] = a & border;
    }
    flood(allowed, reached, h, wpr, &changed);
    for (int64_t e = tid; e < words; e += POST_WG) {              // filled = not reached; kept in the plane of the allowed bits
        const int j = (int)(e % wpr);
        allowed[e] = ~reached[e] & row_mask(w, j);
    }
    __syncthreads();
    for (int64_t k = tid; k < n_words; k += POST_WG) dst[k] = gather_word(allowed, h, w, wpr, k);
    if (tid == 0) F.status[i] = 0;
}

extern "C" hipError_t sdsm_launch_post_fill(int n, const int32_t *dims, const int64_t *off, const uint32_t *in, uint32_t *out, uint32_t *ws,
                                            const int64_t *ws_off, int32_t *status, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    FillParams F{n, dims, off, in, out, ws, ws_off, status};
    hipLaunchKernelGGL(sdsm_k_post_fill, dim3(n), dim3(POST_WG), 0, stream, F);
    return hipGetLastError();
}

// ---- the glare test (superdsm/postprocess.py:269-286) --------------------------------------------------------------------------------
namespace {

struct GlareParams {
    int32_t n_images, num_layers;
    int32_t first[SDSM_MAX_SET_IMAGES + 1];      // prefix of the images' object counts
    sdsm_post_image im[SDSM_MAX_SET_IMAGES];     // d_g: the smoothed glare image; H, W, n_objects
    double props[SDSM_POST_MAX_GLARE_LAYERS];
    const int32_t *boxes;
    const int64_t *bits_off;
    const uint32_t *bits;
    uint32_t *ws;                                // three planes for every fragment beyond POST_FLOOD_WORDS (may be null)
    const int64_t *ws_off;
    int32_t *out;                                // n x 2: pixels of the eroded mask (-1: no workspace, -2: box outside the image), layer bits
};

}  // namespace

__global__ __launch_bounds__(POST_WG) void sdsm_k_post_glare(GlareParams G)
{
    __shared__ uint32_t planes[3 * POST_FLOOD_WORDS];
    __shared__ double dred[POST_WG / 64 * 2];
    __shared__ int ired[POST_WG / 64 * 2], changed;
    const int i = blockIdx.x, tid = threadIdx.x;
    const sdsm_post_image &im = G.im[set_find(G.first, G.n_images, i)];
    const int r0 = G.boxes[4 * i], c0 = G.boxes[4 * i + 1], h = G.boxes[4 * i + 2], w = G.boxes[4 * i + 3], wpr = (w + 31) >> 5;
    if (r0 < 0 || c0 < 0 || h < 1 || w < 1 || r0 + h > im.H || c0 + w > im.W) { if (tid == 0) { G.out[2 * i] = -2; G.out[2 * i + 1] = 0; } return; }
    const int64_t words = (int64_t)h * wpr, n_words = ((int64_t)h * w + 31) >> 5;
    const uint32_t *src = G.bits + G.bits_off[i];
    uint32_t *mask = planes, *layer = planes + POST_FLOOD_WORDS, *reached = planes + 2 * POST_FLOOD_WORDS;
    if (words > POST_FLOOD_WORDS) {
        if (!G.ws || !G.ws_off || G.ws_off[i] < 0) { if (tid == 0) { G.out[2 * i] = -1; G.out[2 * i + 1] = 0; } return; }
        mask = G.ws + G.ws_off[i];
        layer = mask + words;
        reached = layer + words;
    }
    // the fragment, row-packed; outside the fragment counts as foreground (the border does not erode): the bits past w are set
    uint32_t *frag = reached;
    for (int64_t e = tid; e < words; e += POST_WG) {
        const int r = (int)(e / wpr), j = (int)(e - (int64_t)r * wpr);
        frag[e] = load_row_word(src, n_words, w, r, j) | ~row_mask(w, j);
    }
    __syncthreads();
    // erosion by disk(2): the 13 pixels with dy^2 + dx^2 <= 4
    int cnt = 0;
    for (int64_t e = tid; e < words; e += POST_WG) {
        const int r = (int)(e / wpr), j = (int)(e - (int64_t)r * wpr);
        auto word = [&](int rr, int jj) -> uint32_t { return (jj < 0 || jj >= wpr) ? 0xffffffffu : frag[(size_t)rr * wpr + jj]; };
        auto at = [&](int dy, int dx) -> uint32_t {                // bit c: the pixel (r + dy, 32 j + c + dx)
            const int rr = r + dy;
            if (rr < 0 || rr >= h) return 0xffffffffu;
            const uint32_t cur = word(rr, j);
            if (dx == 0) return cur;
            return dx > 0 ? (cur >> dx) | (word(rr, j + 1) << (32 - dx)) : (cur << -dx) | (word(rr, j - 1) >> (32 + dx));
        };
        const uint32_t v = at(0, 0) & at(0, 1) & at(0, -1) & at(0, 2) & at(0, -2) & at(-1, 0) & at(-1, 1) & at(-1, -1) & at(1, 0) & at(1, 1) & at(1, -1) &
                           at(-2, 0) & at(2, 0) & row_mask(w, j);
        mask[e] = v;
        cnt += __popc(v);
    }
    // numpy's max / min of the smoothed intensities over the eroded mask: a NaN among them makes both NaN
    double mn = INFINITY, mx = -INFINITY;
    int has_nan = 0;
    for (int64_t e = tid; e < words; e += POST_WG) {
        const int r = (int)(e / wpr), j = (int)(e - (int64_t)r * wpr);
        for (uint32_t v = mask[e]; v; v &= v - 1) {
            const double gv = im.d_g[(size_t)(r0 + r) * im.W + (c0 + 32 * j + __ffs(v) - 1)];
            if (gv != gv) has_nan = 1;
            else { mn = gv < mn ? gv : mn; mx = gv > mx ? gv : mx; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
        cnt += __shfl_xor(cnt, o); has_nan |= __shfl_xor(has_nan, o);
    }
    __syncthreads();
    if ((tid & 63) == 0) { dred[(tid >> 6) * 2] = mn; dred[(tid >> 6) * 2 + 1] = mx; ired[(tid >> 6) * 2] = cnt; ired[(tid >> 6) * 2 + 1] = has_nan; }
    __syncthreads();
    cnt = 0; has_nan = 0;
    for (int wv = 0; wv < POST_WG / 64; wv++) {
        mn = dred[2 * wv] < mn ? dred[2 * wv] : mn; mx = dred[2 * wv + 1] > mx ? dred[2 * wv + 1] : mx;
        cnt += ired[2 * wv]; has_nan |= ired[2 * wv + 1];
    }
    __syncthreads();
    uint32_t several = 0;
    if (cnt > 0 && !has_nan) {
        for (int l = 0; l < G.num_layers; l++) {
            const double thr = mul_then_add(mx - mn, G.props[l], mn);
            int first = 0x7fffffff;
            for (int64_t e = tid; e < words; e += POST_WG) {
                const int r = (int)(e / wpr), j = (int)(e - (int64_t)r * wpr);
                uint32_t a = 0;
                for (uint32_t v = mask[e]; v; v &= v - 1) {
                    const int c = __ffs(v) - 1;
                    if (im.d_g[(size_t)(r0 + r) * im.W + (c0 + 32 * j + c)] > thr) a |= 1u << c;
                }
                layer[e] = a;
                reached[e] = 0;
                if (a && (int)e < first) first = (int)e;
            }
            first = block_min_i32<POST_WG / 64>(first, ired);
            if (first == 0x7fffffff) continue;                     // an empty layer has no component
            if (tid == 0) reached[first] = layer[first] & (0u - layer[first]);
            flood(layer, reached, h, wpr, &changed);
            int differ = 0;
            for (int64_t e = tid; e < words; e += POST_WG) differ |= layer[e] != reached[e];
            if (-block_min_i32<POST_WG / 64>(-differ, ired)) several |= 1u << l;
            __syncthreads();
        }
    }
    if (tid == 0) { G.out[2 * i] = cnt; G.out[2 * i + 1] = (int32_t)several; }
}

extern "C" hipError_t sdsm_launch_post_glare(const sdsm_post_image *images, int n_images, const int32_t *boxes, const int64_t *bits_off,
                                             const uint32_t *bits, const double *props, int num_layers, uint32_t *ws, const int64_t *ws_off,
                                             int32_t *out, hipStream_t stream)
{
    GlareParams G{};
    G.n_images = n_images; G.num_layers = num_layers;
    G.first[0] = 0;
    for (int j = 0; j < n_images; j++) {
        G.im[j] = images[j];
        G.first[j + 1] = G.first[j] + images[j].n_objects;
    }
    const int n = G.first[n_images];
    if (n <= 0) return hipSuccess;
    for (int l = 0; l < num_layers; l++) G.props[l] = props[l];
    G.boxes = boxes; G.bits_off = bits_off; G.bits = bits; G.ws = ws; G.ws_off = ws_off; G.out = out;
    hipLaunchKernelGGL(sdsm_k_post_glare, dim3(n), dim3(POST_WG), 0, stream, G);
    return hipGetLastError();
}

// ---- the background mask (superdsm/postprocess.py:152-155) ---------------------------------------------------------------------------
// ~(the objects painted in their order) eroded by disk(r), the outside of the image background (the border does not erode), in
// integers: a pixel survives iff for every dy in [-r, r] row y + dy has no covered pixel within floor(sqrt(r^2 - dy^2)) columns.
// fill_foreground ASSIGNS an object's whole box (objects.py:46-52), so where boxes overlap the LAST object decides, also with a
// clear bit: the paint is an atomic maximum of 2 * (object + 1) + bit in an int32 work image, whose low bit is then the cover.
namespace {

struct BgParams {
    int32_t n_images, radius;
    int32_t first_obj[SDSM_MAX_SET_IMAGES + 1];  // prefix of the images' object counts
    int32_t first_wg[SDSM_MAX_SET_IMAGES + 1];   // prefix of the images' tiles of POST_WG pixels
    sdsm_post_bg_image im[SDSM_MAX_SET_IMAGES];
    int8_t reach[SDSM_POST_MAX_BG_RADIUS + 1];   // floor(sqrt(r^2 - dy^2))
    const int32_t *boxes;
    const int64_t *bits_off;
    const uint32_t *bits;
};

}  // namespace

__global__ __launch_bounds__(POST_WG) void sdsm_k_post_bg_paint(BgParams B)
{
    const int i = blockIdx.x;
    const sdsm_post_bg_image &im = B.im[set_find(B.first_obj, B.n_images, i)];
    const int r0 = B.boxes[4 * i], c0 = B.boxes[4 * i + 1], h = B.boxes[4 * i + 2], w = B.boxes[4 * i + 3];
    const uint32_t *bits = B.bits + B.bits_off[i];
    const int64_t total = (int64_t)h * w;
    for (int64_t e = threadIdx.x; e < total; e += POST_WG) {
        const int r = (int)(e / w), c = (int)(e - (int64_t)r * w), y = r0 + r, x = c0 + c;
        if (y < 0 || x < 0 || y >= im.H || x >= im.W) continue;
        atomicMax(&im.d_work[(size_t)y * im.W + x], (int32_t)(2 * (i + 1)) | (int32_t)((bits[e >> 5] >> (e & 31)) & 1u));
    }
}

// dist = columns to the nearest covered pixel of the row, r + 1 beyond r: a uint8 plane of its own behind the H * W work words, so
// that no thread reads a word another one writes.
__global__ __launch_bounds__(POST_WG) void sdsm_k_post_bg_rows(BgParams B)
{
    const int k = set_find(B.first_wg, B.n_images, blockIdx.x);
    const sdsm_post_bg_image &im = B.im[k];
    const int64_t p = (int64_t)(blockIdx.x - B.first_wg[k]) * POST_WG + threadIdx.x;
    if (p >= (int64_t)im.H * im.W) return;
    const int x = (int)(p % im.W);
    const int32_t *row = im.d_work + (p - x);
    const int cover = row[x] & 1;
    int d = 0;
    if (!cover) {
        for (d = 1; d <= B.radius; d++)
            if ((x - d >= 0 && (row[x - d] & 1)) || (x + d < im.W && (row[x + d] & 1))) break;
    }
    ((uint8_t *)(im.d_work + (int64_t)im.H * im.W))[p] = (uint8_t)d;
}

__global__ __launch_bounds__(POST_WG) void sdsm_k_post_bg_erode(BgParams B)
{
    const int k = set_find(B.first_wg, B.n_images, blockIdx.x);
    const sdsm_post_bg_image &im = B.im[k];
    const int64_t p = (int64_t)(blockIdx.x - B.first_wg[k]) * POST_WG + threadIdx.x;
    if (p >= (int64_t)im.H * im.W) return;
    const int y = (int)(p / im.W);
    const uint8_t *dist = (const uint8_t *)(im.d_work + (int64_t)im.H * im.W);
    bool keep = true;
    for (int dy = -B.radius; dy <= B.radius && keep; dy++) {
        if (y + dy < 0 || y + dy >= im.H) continue;
        keep = dist[p + (int64_t)dy * im.W] > B.reach[dy < 0 ? -dy : dy];
    }
    im.d_bg[p] = keep ? 1 : 0;
}

extern "C" hipError_t sdsm_launch_post_background(const sdsm_post_bg_image *images, int n_images, const int32_t *boxes, const int64_t *bits_off,
                                                  const uint32_t *bits, int radius, hipStream_t stream)
{
    BgParams B{};
    B.n_images = n_images; B.radius = radius;
    for (int j = 0; j < n_images; j++) {
        B.im[j] = images[j];
        B.first_obj[j + 1] = B.first_obj[j] + images[j].n_objects;
        B.first_wg[j + 1] = B.first_wg[j] + (int32_t)(((int64_t)images[j].H * images[j].W + POST_WG - 1) / POST_WG);
        hipError_t e = hipMemsetAsync(images[j].d_work, 0, sizeof(int32_t) * (size_t)images[j].H * images[j].W, stream);
        if (e != hipSuccess) return e;
    }
    for (int dy = 0; dy <= radius; dy++) {
        int c = 0;
        while ((c + 1) * (c + 1) + dy * dy <= radius * radius) c++;
        B.reach[dy] = (int8_t)c;
    }
    B.boxes = boxes; B.bits_off = bits_off; B.bits = bits;
    if (B.first_obj[n_images] > 0) hipLaunchKernelGGL(sdsm_k_post_bg_paint, dim3(B.first_obj[n_images]), dim3(POST_WG), 0, stream, B);
    hipLaunchKernelGGL(sdsm_k_post_bg_rows, dim3(B.first_wg[n_images]), dim3(POST_WG), 0, stream, B);
    hipLaunchKernelGGL(sdsm_k_post_bg_erode, dim3(B.first_wg[n_images]), dim3(POST_WG), 0, stream, B);
    return hipGetLastError();
}
