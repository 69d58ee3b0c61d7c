// Intensity distribution tables on the GPU: one sdsm_intensity_record per object (bit-packed fragments) or per label (the windows of
// sdsm_shape.hip) and the two order statistics of every quantile, for one image or a set of images.  No reference counterpart; the
// definition the kernel is tested against is the host code of superdsm_amd/intensity.py.
//
//   k_intensity_objects   one workgroup of 256 threads per fragment, which walks the fragment's set bits (each_set_bit of sdsm_tables.h).
//     pass A      area, bounding box, n_finite, the monotone keys of gmin and gmax, the flags; every finite pixel's key goes to LDS while
//                 there is room (the place by an LDS integer add: the order of the keys does not matter to a selection)
//     pass B      from gmin and range_exp the three integer sums, in registers, then one shuffle and one LDS reduction
//     selection   an exact radix select on the 64-bit key, 8-bit digits from the top: a round builds a 256-bin histogram in LDS over the
//                 keys that share the prefix found so far, one wavefront scans it, picks the bin of the rank and subtracts what lies
//                 below; after the last digit the prefix is the key, and the last bin's count says how many keys equal it.  The rank
//                 above is then either the same key or, by one more pass, the smallest key above it: no second selection.
//     MAD         the same routine on the keys of |g - med|
//   An object with at most SDSM_INTENSITY_LDS_KEYS finite pixels is selected from its keys in LDS (rewritten in place for the MAD); a
//   larger one walks its fragment and re-reads d_g in every round: the same bytes, more slowly.
// No float atomics, no global atomics, no output that needs clearing.
#include "sdsm_tables.h"
#include "sdsm_quantile.h"
#include <climits>

namespace {

constexpr int ITPB = 256;                        // threads of a workgroup = bins of a histogram
constexpr int KCAP = SDSM_INTENSITY_LDS_KEYS;
constexpr int NQ = SDSM_INTENSITY_MAX_QUANTILES;
constexpr int IWAVES = ITPB / 64;

struct IQuant {                                  // the quantiles of a launch
    int32_t n_q;
    int32_t num[NQ], den[NQ];
};

struct ILds {
    u64 keys[KCAP];
    uint32_t hist[ITPB];
    u64 r64[IWAVES][4];
    int32_t r32[IWAVES][6];
    uint32_t count;                              // finite pixels seen by pass A (the first KCAP of them are in keys)
    uint32_t sel_bin, sel_r, sel_cnt;
};

struct Src {                                     // where the keys of the object come from
    const uint32_t *bits;
    const double *g;
    Fragment box;
    uint32_t n;                                  // staged keys
    bool staged, mad;
    double med;
};

// 0.5 a + 0.5 b as two products and one sum.  Contraction is switched off for these statements: a fused multiply-add rounds once where
// this rounds twice, which shows for subnormals (the compiler contracts __dadd_rn(__dmul_rn(..), ..) as well: they are plain operators).
__device__ __forceinline__ double midpoint(double a, double b)
{
#pragma clang fp contract(off)
    const double x = 0.5 * a, y = 0.5 * b;
    return x + y;
}

// f(row, column, g) for every set bit of the fragment
template <class F>
__device__ __forceinline__ void each_pixel(const Src &s, int tid, F f)
{
    each_set_bit<ITPB>(s.bits, s.box, tid, [&](uint32_t, int r, int c) { f(r, c, s.g[(int64_t)r * s.box.W + c]); });
}

// f(key) for every key of the object: of g, or of |g - med| once the MAD is being taken
template <class F>
__device__ __forceinline__ void each_key(const Src &s, const u64 *keys, int tid, F f)
{
    if (s.staged) {
        for (uint32_t k = tid; k < s.n; k += ITPB) f(keys[k]);
    } else {
        each_pixel(s, tid, [&](int, int, double g) {
            if (finite_bits(g)) f(s.mad ? dkey(fabs(g - s.med)) : dkey(g));
        });
    }
}

// The key at rank r (from 0) of the object's keys; below: keys smaller than it, eq: keys equal to it.  r is the same in every thread
// and smaller than the number of keys.
__device__ __forceinline__ u64 radix_select(const Src &s, ILds &T, int tid, uint32_t r, uint32_t &below, uint32_t &eq)
{
    u64 prefix = 0;
    const uint32_t rank = r;
    for (int shift = 56; shift >= 0; shift -= 8) {
        T.hist[tid] = 0;
        __syncthreads();
        const u64 above = shift == 56 ? 0ull : ~0ull << (shift + 8);             // the digits already fixed
        each_key(s, T.keys, tid, [&](u64 k) {
            if ((k & above) == prefix) atomicAdd(&T.hist[(uint32_t)(k >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (tid < 64) select_bin(T.hist, tid, r, T.sel_bin, T.sel_r, T.sel_cnt);     // one wavefront
        __syncthreads();
        prefix |= (u64)T.sel_bin << shift;
        r = T.sel_r;
        eq = T.sel_cnt;
    }
    below = rank - r;
    return prefix;
}

// the smallest key above `key` (there is one)
__device__ __forceinline__ u64 next_above(const Src &s, ILds &T, int tid, u64 key)
{
    u64 m = ~0ull;                               // (no key: the largest is that of +inf)
    each_key(s, T.keys, tid, [&](u64 k) { if (k > key && k < m) m = k; });
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_down(m, o); m = t < m ? t : m; }
    __syncthreads();                             // (r64 may still be read from the reduction before)
    if ((tid & 63) == 0) T.r64[tid >> 6][0] = m;
    __syncthreads();
    m = T.r64[0][0];
    for (int k = 1; k < IWAVES; k++) m = T.r64[k][0] < m ? T.r64[k][0] : m;
    return m;
}

// the order statistics at the two ranks of the quantile num / den of the object's n keys
__device__ __forceinline__ void order_pair(const Src &s, ILds &T, int tid, i64 n, int32_t num, int32_t den, double &v_lo, double &v_hi)
{
    int64_t lo, hi, rem;
    sdsm_quantile_ranks_inline(n, num, den, &lo, &hi, &rem);
    uint32_t below, eq;
    const u64 k_lo = radix_select(s, T, tid, (uint32_t)lo, below, eq);
    u64 k_hi = k_lo;
    if (hi != lo && (uint32_t)lo - below + 1 >= eq) k_hi = next_above(s, T, tid, k_lo);          // rank lo is the last of its equals
    v_lo = dkey_inv(k_lo); v_hi = dkey_inv(k_hi);
}

__device__ __forceinline__ void empty_result(sdsm_intensity_record *out, double *order, int n_q, i64 area, int flags)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    sdsm_intensity_record R;
    R.area = area; R.n_finite = 0; R.sum_p = 0; R.sum_pp_lo = R.sum_pp_hi = 0;
    R.gmin = __longlong_as_double(0x7ff0000000000000ll); R.gmax = __longlong_as_double((i64)0xfff0000000000000ull);
    R.med_lo = R.med_hi = R.mad_lo = R.mad_hi = nan;
    R.range_exp = 0; R.flags = flags | 4;
    *out = R;
    for (int q = 0; q < 2 * n_q; q++) order[q] = nan;
}

__global__ __launch_bounds__(ITPB) void k_intensity_objects(SetImages S, IQuant Q, const int32_t *obj_image, const int32_t *boxes, const int64_t *bits_off,
                                                            const uint32_t *bits_, const double *g_, sdsm_intensity_record *out, double *order_)
{
    __shared__ ILds T;
    const int i = blockIdx.x, tid = threadIdx.x;
    double *order = order_ + (int64_t)i * Q.n_q * 2;
    const int im = obj_image ? obj_image[i] : 0;
    const bool im_ok = im >= 0 && im < S.n;
    const int H = im_ok ? S.H[im] : 0, W = im_ok ? S.W[im] : 0;
    const int br0 = boxes[4 * i], bc0 = boxes[4 * i + 1], h = boxes[4 * i + 2], w = boxes[4 * i + 3];
    // (fragment_box of sdsm_tables.h, written out: see "What the table kernels share" in DESIGN.md)
    if (!(im_ok && br0 >= 0 && bc0 >= 0 && h >= 1 && w >= 1 && h <= H && w <= W && br0 <= H - h && bc0 <= W - w)) {
        if (tid == 0) empty_result(out + i, order, Q.n_q, 0, 0);                 // (uniform: the whole workgroup leaves; nothing is read)
        return;
    }
    Src s;
    s.box = {H, W, br0, bc0, h, w};
    s.bits = bits_ + bits_off[i];
    s.g = g_ + S.off[im];
    s.staged = false; s.mad = false; s.med = 0.0; s.n = 0;
    if (tid == 0) T.count = 0;
    __syncthreads();

    // ---- pass A --------------------------------------------------------------------------------------------------------------------
    uint32_t area = 0, nfin = 0;
    int flags = 0, r0 = INT_MAX, c0 = INT_MAX, r1 = 0, c1 = 0;
    u64 kmin = ~0ull, kmax = 0;
    each_pixel(s, tid, [&](int r, int c, double g) {
        area++;
        r0 = r < r0 ? r : r0; r1 = r + 1 > r1 ? r + 1 : r1;
        c0 = c < c0 ? c : c0; c1 = c + 1 > c1 ? c + 1 : c1;
        if (!finite_bits(g)) { flags |= 2; return; }
        nfin++;
        const u64 k = dkey(g);
        kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax;
        const uint32_t pos = atomicAdd(&T.count, 1u);
        if (pos < (uint32_t)KCAP) T.keys[pos] = k;
    });
    for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_down(area, o); nfin += __shfl_down(nfin, o); flags |= __shfl_down(flags, o);
        const u64 a = __shfl_down(kmin, o), b = __shfl_down(kmax, o);
        kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
        const int t0 = __shfl_down(r0, o), t1 = __shfl_down(c0, o), t2 = __shfl_down(r1, o), t3 = __shfl_down(c1, o);
        r0 = t0 < r0 ? t0 : r0; c0 = t1 < c0 ? t1 : c0; r1 = t2 > r1 ? t2 : r1; c1 = t3 > c1 ? t3 : c1;
    }
    if ((tid & 63) == 0) {
        const int wv = tid >> 6;
        T.r64[wv][0] = area; T.r64[wv][1] = nfin; T.r64[wv][2] = kmin; T.r64[wv][3] = kmax;
        T.r32[wv][0] = flags; T.r32[wv][1] = r0; T.r32[wv][2] = c0; T.r32[wv][3] = r1; T.r32[wv][4] = c1;
    }
    __syncthreads();
    i64 n_area = 0, n = 0;
    kmin = ~0ull; kmax = 0; flags = 0; r0 = c0 = INT_MAX; r1 = c1 = 0;
    for (int k = 0; k < IWAVES; k++) {           // every thread: the same values
        n_area += (i64)T.r64[k][0]; n += (i64)T.r64[k][1];
        kmin = T.r64[k][2] < kmin ? T.r64[k][2] : kmin; kmax = T.r64[k][3] > kmax ? T.r64[k][3] : kmax;
        flags |= T.r32[k][0];
        r0 = T.r32[k][1] < r0 ? T.r32[k][1] : r0; c0 = T.r32[k][2] < c0 ? T.r32[k][2] : c0;
        r1 = T.r32[k][3] > r1 ? T.r32[k][3] : r1; c1 = T.r32[k][4] > c1 ? T.r32[k][4] : c1;
    }
    if (n_area > 0 && (r0 == 0 || c0 == 0 || r1 == H || c1 == W)) flags |= 1;
    if (n == 0) {
        if (tid == 0) empty_result(out + i, order, Q.n_q, n_area, flags);
        return;
    }
    s.staged = n <= KCAP;
    s.n = s.staged ? (uint32_t)n : 0;

    // ---- pass B --------------------------------------------------------------------------------------------------------------------
    const double gmin = dkey_inv(kmin), gmax = dkey_inv(kmax);
    const double d = gmax - gmin;
    int e = 0;
    if (!finite_bits(d)) { flags |= 8; e = 1024; }
    else if (d != 0.0) {
        const int E = (int)(((u64)__double_as_longlong(d) >> 52) & 0x7ff);
        e = E == 0 ? -960 : E - 1022;
        e = e < -960 ? -960 : e;
    }
    i64 sum_p = 0;
    u64 pp_lo = 0, pp_hi = 0;
    if (!(flags & 8)) {
        each_key(s, T.keys, tid, [&](u64 k) {
            const u64 p = (u64)(i64)rint(ldexp(dkey_inv(k) - gmin, 30 - e));     // 0 <= p <= 2^30
            const u64 pp = p * p;
            sum_p += (i64)p; pp_lo += pp & 0xffffffffull; pp_hi += pp >> 32;
        });
        for (int o = 32; o > 0; o >>= 1) { sum_p += __shfl_down(sum_p, o); pp_lo += __shfl_down(pp_lo, o); pp_hi += __shfl_down(pp_hi, o); }
    }
    __syncthreads();                             // r64 has been read by everyone
    if ((tid & 63) == 0) { T.r64[tid >> 6][0] = (u64)sum_p; T.r64[tid >> 6][1] = pp_lo; T.r64[tid >> 6][2] = pp_hi; }
    __syncthreads();
    sum_p = 0; pp_lo = pp_hi = 0;
    for (int k = 0; k < IWAVES; k++) { sum_p += (i64)T.r64[k][0]; pp_lo += T.r64[k][1]; pp_hi += T.r64[k][2]; }

    // ---- the quantiles, the median, the MAD ----------------------------------------------------------------------------------------
    double m_lo = 0.0, m_hi = 0.0, med_lo = 0.0, med_hi = 0.0;
    for (int q = 0; q < Q.n_q + 2; q++) {        // the caller's quantiles, then the median of g, then that of |g - med|
        const bool named = q < Q.n_q;
        if (q == Q.n_q + 1) {
            med_lo = m_lo; med_hi = m_hi;
            s.med = midpoint(m_lo, m_hi);
            s.mad = true;
            if (s.staged) {
                for (uint32_t k = tid; k < s.n; k += ITPB) T.keys[k] = dkey(fabs(dkey_inv(T.keys[k]) - s.med));
                __syncthreads();
            }
        }
        double v_lo, v_hi;
        order_pair(s, T, tid, n, named ? Q.num[q] : 1, named ? Q.den[q] : 2, v_lo, v_hi);
        if (!named) { m_lo = v_lo; m_hi = v_hi; }
        else if (tid == 0) { order[2 * q] = v_lo; order[2 * q + 1] = v_hi; }
    }
    if (tid == 0) {
        sdsm_intensity_record R;
        R.area = n_area; R.n_finite = n; R.sum_p = sum_p; R.sum_pp_lo = pp_lo; R.sum_pp_hi = pp_hi;
        R.gmin = gmin; R.gmax = gmax; R.med_lo = med_lo; R.med_hi = med_hi; R.mad_lo = m_lo; R.mad_hi = m_hi;
        R.range_exp = e; R.flags = flags;
        out[i] = R;
    }
}

}  // namespace

extern "C" hipError_t sdsm_intensity_objects_impl(const sdsm_set_image *images, int n_images, int n, const int32_t *obj_image, const int32_t *boxes,
                                                  const int64_t *bits_off, const uint32_t *bits, const double *d_g, int n_q, const int32_t *num,
                                                  const int32_t *den, sdsm_intensity_record *out, double *order, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const SetImages S = make_set(images, n_images);
    IQuant Q{};
    Q.n_q = n_q;
    for (int q = 0; q < n_q; q++) { Q.num[q] = num[q]; Q.den[q] = den[q]; }
    hipLaunchKernelGGL(k_intensity_objects, dim3(n), dim3(ITPB), 0, stream, S, Q, obj_image, boxes, bits_off, bits, d_g, out, order);
    return hipGetLastError();
}
