// Host-side combinatorial steps of the global-energy-minimisation stage as native code (no device access): the approximate
// min-weight set cover (reference: superdsm/minsetcover.py:4-88, Algorithm 2 of Kostrykin & Rohr, TPAMI 2023) and the greedy
// max-weight set packing (superdsm/maxsetpack.py:8-24).  They stay on the host by design (BASELINE.json north_star); once the
// candidate solves run on the GPU the Python loops of the set cover are the largest part of the stage's wall clock per image.
// Same decisions as the Python restatement in superdsm_amd/minsetcover.py / maxsetpack.py, which follows the reference: same
// arithmetic (IEEE double, same order of the sums), same tie-breaking (first minimum / maximum in list order, stable sort).
// Footprints are bit sets over the atoms of one cluster: `words` uint64 per object.
#include <algorithm>
#include <cstdint>
#include <functional>
#include <queue>
#include <tuple>
#include <unordered_set>
#include <vector>

#include "../../include/sdsm.h"
#include "sdsm_quantile.h"
#include "sdsm_neighbours.h"
#include "sdsm_texture.h"
#include "sdsm_depth.h"
#include "sdsm_parts.h"
#include "sdsm_skeleton.h"

namespace {

struct Family {
    int n, words;
    const uint64_t *foot;
    const double *energy;
    const uint64_t *fp(int i) const { return foot + (size_t)i * words; }
};

inline int popcount_and(const uint64_t *a, const uint64_t *b, int words)
{
    int c = 0;
    for (int w = 0; w < words; w++) c += __builtin_popcountll(a[w] & b[w]);
    return c;
}
inline bool disjoint(const uint64_t *a, const uint64_t *b, int words)
{
    for (int w = 0; w < words; w++) if (a[w] & b[w]) return false;
    return true;
}
inline bool subset(const uint64_t *a, const uint64_t *b, int words)   // a <= b
{
    for (int w = 0; w < words; w++) if (a[w] & ~b[w]) return false;
    return true;
}

// greedy phase + merge phase for one beta (minsetcover.py:24-50)
std::vector<int> solve_once(const Family &F, double beta, bool merge)
{
    const int W = F.words;
    std::vector<uint64_t> uncovered(W, 0);
    for (int i = 0; i < F.n; i++) for (int w = 0; w < W; w++) uncovered[w] |= F.fp(i)[w];
    std::vector<int> cand(F.n), accepted;
    for (int i = 0; i < F.n; i++) cand[i] = i;
    while (!cand.empty()) {
        int best = -1;
        double best_price = 0;
        for (int c : cand) {
            const double price = (F.energy[c] + beta) / popcount_and(F.fp(c), uncovered.data(), W);
            if (best < 0 || price < best_price) { best = c; best_price = price; }     // first minimum in list order
        }
        accepted.push_back(best);
        for (int w = 0; w < W; w++) uncovered[w] &= ~F.fp(best)[w];
        std::vector<int> rest;
        for (int c : cand) if (!disjoint(F.fp(c), uncovered.data(), W)) rest.push_back(c);
        cand.swap(rest);
    }
    if (!merge) return accepted;
    std::vector<char> taken(F.n, 0);
    for (int a : accepted) taken[a] = 1;
    std::vector<int> others;
    for (int i = 0; i < F.n; i++) if (!taken[i]) others.push_back(i);
    std::stable_sort(others.begin(), others.end(), [&](int a, int b) { return F.energy[a] + beta < F.energy[b] + beta; });
    for (int nw : others) {
        std::vector<int> inside;
        bool valid = true;
        for (int c : accepted) {
            if (disjoint(F.fp(c), F.fp(nw), W)) continue;
            if (!subset(F.fp(c), F.fp(nw), W)) { valid = false; break; }           // partial overlap: not a valid replacement
            inside.push_back(c);
        }
        if (!valid) continue;
        double sum = 0;                                                             // Python's sum(): left to right from 0
        for (int c : inside) sum += F.energy[c] + beta;
        if (F.energy[nw] + beta < sum) {
            std::vector<int> next;
            for (int c : accepted) if (std::find(inside.begin(), inside.end(), c) == inside.end()) next.push_back(c);
            next.push_back(nw);
            accepted.swap(next);
        }
    }
    return accepted;
}

double price_of(const Family &F, const std::vector<int> &sol, double beta)
{
    double s = 0;
    for (int c : sol) s += F.energy[c];
    return s + beta * (double)sol.size();
}

std::vector<int> solve_cover(const Family &F, double beta, bool merge, int max_iter, double gamma)
{
    std::vector<int> solution = solve_once(F, beta, merge);
    if (max_iter > 1 && beta > 0) {
        std::vector<int> retry = solve_cover(F, beta * gamma, merge, max_iter - 1, gamma);
        if (price_of(F, retry, beta) < price_of(F, solution, beta)) return retry;   // priced with the beta of THIS level
    }
    return solution;
}

}  // namespace

extern "C" int sdsm_minsetcover(int n, int words, const uint64_t *footprints, const double *energies, double beta, int merge, int max_iter,
                                double gamma, int32_t *selected, int32_t *n_selected)
{
    if (n < 0 || words < 1 || !selected || !n_selected || (n > 0 && (!footprints || !energies)) || !(beta >= 0) || !(gamma > 0 && gamma < 1)) return SDSM_ERR_ARGUMENT;
    Family F{n, words, footprints, energies};
    std::vector<int> sol = n > 0 ? solve_cover(F, beta, merge != 0, max_iter, gamma) : std::vector<int>();
    *n_selected = (int32_t)sol.size();
    for (size_t i = 0; i < sol.size(); i++) selected[i] = sol[i];
    return SDSM_OK;
}

// The same for SEVERAL independent families in one call (MinSetCover.update: one cover per touched cluster and generation -- a hundred
// calls per image, each paying the trip through the foreign-function interface): family f has n[f] objects of words[f] uint64 each, its
// footprints / energies / selected indices start at the running sums of n[f] * words[f] / n[f] / n[f].
extern "C" int sdsm_minsetcover_multi(int n_families, const int32_t *n, const int32_t *words, const uint64_t *footprints, const double *energies, double beta,
                                      int merge, int max_iter, double gamma, int32_t *selected, int32_t *n_selected)
{
    if (n_families < 0 || (n_families > 0 && (!n || !words || !footprints || !energies || !selected || !n_selected)) || !(beta >= 0) || !(gamma > 0 && gamma < 1)) return SDSM_ERR_ARGUMENT;
    size_t fo = 0, eo = 0;
    for (int f = 0; f < n_families; f++) {
        if (n[f] < 0 || words[f] < 1) return SDSM_ERR_ARGUMENT;
        Family F{n[f], words[f], footprints + fo, energies + eo};
        std::vector<int> sol = n[f] > 0 ? solve_cover(F, beta, merge != 0, max_iter, gamma) : std::vector<int>();
        n_selected[f] = (int32_t)sol.size();
        for (size_t i = 0; i < sol.size(); i++) selected[eo + i] = sol[i];
        fo += (size_t)n[f] * words[f];
        eo += (size_t)n[f];
    }
    return SDSM_OK;
}

extern "C" int sdsm_maxsetpack(int n, int words, const uint64_t *footprints, const double *energies, int32_t *selected, int32_t *n_selected)
{
    if (n < 0 || words < 1 || !selected || !n_selected || (n > 0 && (!footprints || !energies))) return SDSM_ERR_ARGUMENT;
    Family F{n, words, footprints, energies};
    std::vector<int> pool(n), packed;
    for (int i = 0; i < n; i++) pool[i] = i;
    while (!pool.empty()) {
        int top = pool[0];
        for (int c : pool) if (energies[c] > energies[top]) top = c;                 // first maximum in list order
        packed.push_back(top);
        std::vector<int> rest;
        for (int c : pool) if (disjoint(F.fp(c), F.fp(top), words)) rest.push_back(c);
        pool.swap(rest);
    }
    *n_selected = (int32_t)packed.size();
    for (size_t i = 0; i < packed.size(); i++) selected[i] = packed[i];
    return SDSM_OK;
}

// Size of the search space of the iterations (globalenergymin.py:292-323, _estimate_progress from the atoms on): for every cluster
// the number of footprints that growing the single atoms by one adjacent atom at a time produces, generation after generation
// (de-duplicated within a generation) -- the connected atom subsets of 2 .. n atoms (n - 1 with skip_last: the universe is computed
// separately) whose atoms are pairwise compatible (seed distance).  Atoms of cluster k are offsets[k] .. offsets[k + 1] - 1; adj /
// compat hold, per atom, the bit set of its neighbours / of the atoms it may share a footprint with, as LOCAL bit indices of its
// cluster (compat == NULL: all).  Clusters of more than 64 atoms get -1 (the caller enumerates them itself).  Stops counting once the
// total exceeds max_amount (the caller raises, as the reference does).
extern "C" int sdsm_count_growth(int n_clusters, const int32_t *offsets, const uint64_t *adj, const uint64_t *compat, int skip_last,
                                 int64_t max_amount, int64_t *counts)
{
    if (n_clusters < 0 || !offsets || !counts || (n_clusters > 0 && !adj)) return SDSM_ERR_ARGUMENT;
    int64_t total = 0;
    for (int k = 0; k < n_clusters; k++) {
        const int lo = offsets[k], n = offsets[k + 1] - lo;
        if (n > 64) { counts[k] = -1; continue; }
        counts[k] = 0;
        std::vector<uint64_t> current(n);
        for (int a = 0; a < n; a++) current[a] = 1ull << a;
        int size = 1;
        while (!current.empty() && total <= max_amount) {
            if (skip_last && size + 1 == n) break;                               // no footprint of this generation is grown
            std::unordered_set<uint64_t> next;
            for (uint64_t fp : current) {
                uint64_t nb = 0;
                for (uint64_t m = fp; m; m &= m - 1) nb |= adj[lo + __builtin_ctzll(m)];
                nb &= ~fp;
                for (uint64_t m = nb; m; m &= m - 1) {
                    const int a = __builtin_ctzll(m);
                    if (compat && (compat[lo + a] & fp) != fp) continue;
                    next.insert(fp | (1ull << a));
                }
            }
            counts[k] += (int64_t)next.size();
            total += (int64_t)next.size();
            current.assign(next.begin(), next.end());
            size++;
        }
    }
    return SDSM_OK;
}

// Marker flood of the coarse-to-fine region analysis (the restated rule of scikit-image's heap flood): priority = the
// pixel's own value, ties by push age, then by raster index (markers only: they all have age 0).
extern "C" int sdsm_watershed(const double *image, const int32_t *markers, const uint8_t *mask, int H, int W, int32_t *out)
{
    if (!image || !markers || !out || H < 1 || W < 1 || (int64_t)H * W >= INT32_MAX) return SDSM_ERR_ARGUMENT;
    typedef std::tuple<double, int64_t, int32_t> Entry;
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    const int32_t n = H * W;
    for (int32_t p = 0; p < n; p++) {
        const bool ok = !mask || mask[p];
        out[p] = ok ? markers[p] : 0;
        if (ok && markers[p] != 0) heap.emplace(image[p], 0, p);
    }
    int64_t age = 0;
    while (!heap.empty()) {
        const int32_t p = std::get<2>(heap.top());
        heap.pop();
        const int r = p / W, c = p - r * W;
        const int32_t nb[4] = {r > 0 ? p - W : -1, c > 0 ? p - 1 : -1, c + 1 < W ? p + 1 : -1, r + 1 < H ? p + W : -1};
        for (int32_t q : nb) {
            if (q < 0 || out[q] != 0 || (mask && !mask[q])) continue;
            out[q] = out[p];
            heap.emplace(image[q], ++age, q);
        }
    }
    return SDSM_OK;
}

// The flood of rasterize_labels (superdsm/render.py:432-433 through superdsm_amd/render.py:_watershed) on the sparse set of pixels it
// can touch: n entries in ascending raster index; label > 0: a marker pixel next to an overlap pixel (a seed), label == 0: an overlap
// pixel.  The seeds enter the heap in raster order with ages 0, 1, 2, ...; the heap pops the smallest (distance, age, row, column); a
// popped pixel labels its unlabelled neighbours up, down, left, right, which enter with the next ages.  NOT the rule of
// sdsm_watershed above (all markers age 0; up, left, right, down).
extern "C" int sdsm_flood_sparse(int64_t n, const int32_t *idx, const int32_t *label, const double *dist, int H, int W, int32_t *out)
{
    if (n < 0 || H < 1 || W < 1 || (int64_t)H * W >= INT32_MAX || (n > 0 && (!idx || !label || !dist || !out))) return SDSM_ERR_ARGUMENT;
    for (int64_t k = 0; k < n; k++) {
        if (idx[k] < 0 || idx[k] >= H * W || (k > 0 && idx[k] <= idx[k - 1]) || label[k] < 0) return SDSM_ERR_ARGUMENT;
        out[k] = label[k];
    }
    typedef std::tuple<double, int64_t, int32_t, int32_t> Entry;     // distance, age, raster index (= row, column order), entry
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    int64_t age = 0;
    for (int64_t k = 0; k < n; k++) if (label[k] > 0) heap.emplace(dist[k], age++, idx[k], (int32_t)k);
    const int32_t *end = idx + n;
    while (!heap.empty()) {
        const int32_t p = std::get<2>(heap.top()), k = std::get<3>(heap.top());
        heap.pop();
        const int r = p / W, c = p - r * W;
        const int32_t nb[4] = {r > 0 ? p - W : -1, r + 1 < H ? p + W : -1, c > 0 ? p - 1 : -1, c + 1 < W ? p + 1 : -1};
        for (int32_t q : nb) {
            if (q < 0) continue;
            const int32_t *it = std::lower_bound(idx, end, q);
            if (it == end || *it != q) continue;                     // not in the set: background, or a marker that nothing can change
            const int64_t j = it - idx;
            if (out[j] != 0) continue;
            out[j] = out[k];
            heap.emplace(dist[j], age++, q, (int32_t)j);
        }
    }
    return SDSM_OK;
}

// The ranks of the quantile num / den of n sorted values, as the intensity kernels take them (sdsm_quantile.h: the same inline function).
extern "C" int sdsm_quantile_ranks(int64_t n, int32_t num, int32_t den, int64_t *lo, int64_t *hi, int64_t *rem)
{
    if (n < 1 || n > INT32_MAX || den < 1 || den > SDSM_INTENSITY_MAX_DEN || num < 0 || num > den || !lo || !hi || !rem) return SDSM_ERR_ARGUMENT;
    sdsm_quantile_ranks_inline(n, num, den, lo, hi, rem);
    return SDSM_OK;
}

// The level of a value and the place of a cell, as the texture kernels take them (sdsm_texture.h: the same inline functions).
extern "C" int sdsm_texture_level(const double *edges, int n_edges, double g)
{
    if (n_edges < 0 || n_edges > SDSM_TEXTURE_MAX_LEVELS - 1 || (n_edges > 0 && !edges) || !(g - g == 0)) return -1;
    return sdsm_texture_level_inline(edges, n_edges, g);
}

extern "C" int sdsm_texture_cell(int levels, int i, int j)
{
    if (levels < 1 || levels > SDSM_TEXTURE_MAX_LEVELS || i < 0 || j < i || j >= levels) return -1;
    return sdsm_texture_cell_inline(levels, i, j);
}

// The shell of a squared depth, as the depth kernel takes it (sdsm_depth.h: the same inline function), and the workspace of a box.
static_assert(SDSM_DEPTH_MAX_SHELLS == SDSM_DEPTH_MAX_SHELLS_INLINE, "the limit of the header and of the inline helper");

extern "C" int sdsm_depth_shell(int64_t d2, int n_shells)
{
    if (d2 < 1 || d2 > INT32_MAX || n_shells < 1 || n_shells > SDSM_DEPTH_MAX_SHELLS) return -1;
    return sdsm_depth_shell_inline((int32_t)d2, n_shells);
}

extern "C" int64_t sdsm_depth_workspace_pixels(int h, int w)
{
    if (h < 1 || w < 1) return 0;
    const int64_t px = (int64_t)h * w;
    return px > SDSM_DEPTH_LDS_PIXELS ? px : 0;
}

// The removal rule, the workspace of a box and the thinning of one window, by the word functions the skeleton kernel uses
// (sdsm_skeleton.h: the same inline functions).
static_assert(SDSM_SKELETON_LDS_WORDS == SDSM_SKELETON_LDS_WORDS_INLINE, "the limit of the header and of the inline helper");

extern "C" int sdsm_skeleton_deletable(int code, int direction)
{
    return sdsm_skeleton_deletable_inline(code, direction);
}

extern "C" int64_t sdsm_skeleton_workspace_words(int h, int w)
{
    if (h < 1 || w < 1) return 0;
    const int64_t words = (int64_t)h * (((int64_t)w + 63) / 64);
    return (h <= 64 && w <= 64) || words <= SDSM_SKELETON_LDS_WORDS ? 0 : 2 * words;
}

extern "C" int sdsm_skeleton_thin(int h, int w, const uint32_t *bits, uint32_t *skeleton)
{
    if (h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31) || !bits || !skeleton) return -1;
    const uint32_t n_bits = (uint32_t)h * (uint32_t)w, n32 = (n_bits + 31) >> 5;
    const int nw = (w + 63) / 64;
    std::vector<sdsm_skel_word> A((size_t)h * nw), B((size_t)h * nw);
    for (int r = 0; r < h; r++)
        for (int j = 0; j < nw; j++)
            A[(size_t)r * nw + j] = sdsm_skeleton_flat_bits(bits, n32, (uint32_t)r * (uint32_t)w + 64u * (uint32_t)j, w - 64 * j < 64 ? w - 64 * j : 64);
    const int dirs[4] = {0, 4, 2, 6};
    int cycles = 0;
    for (;;) {
        bool removed = false;
        for (int d : dirs) {
            for (int r = 0; r < h; r++)
                for (int j = 0; j < nw; j++) {
                    const sdsm_skel_word *p = &A[(size_t)r * nw + j];
                    const bool l = j > 0, rt = j + 1 < nw, u = r > 0, dn = r + 1 < h;
                    const sdsm_skel_word up[3] = {u && l ? p[-nw - 1] : 0, u ? p[-nw] : 0, u && rt ? p[-nw + 1] : 0};
                    const sdsm_skel_word row[3] = {l ? p[-1] : 0, p[0], rt ? p[1] : 0};
                    const sdsm_skel_word down[3] = {dn && l ? p[nw - 1] : 0, dn ? p[nw] : 0, dn && rt ? p[nw + 1] : 0};
                    sdsm_skel_word n[8];
                    sdsm_skeleton_planes(up, row, down, n);
                    const sdsm_skel_word rm = sdsm_skeleton_remove(row[1], n, d);
                    B[(size_t)r * nw + j] = row[1] & ~rm;
                    removed |= rm != 0;
                }
            A.swap(B);
        }
        if (!removed) break;
        cycles++;
    }
    for (uint32_t k = 0; k < n32; k++) skeleton[k] = sdsm_skeleton_flat_word(A.data(), (uint32_t)w, (uint32_t)nw, n_bits, k);
    return cycles;
}

// The half-width of a row of the disk and the first probe position of a pair, as the neighbourhood kernel takes them (sdsm_neighbours.h:
// the same inline functions).
static_assert(SDSM_NEIGHBOUR_MAX_D2 == SDSM_NEIGHBOUR_MAX_D2_INLINE, "the limit of the header and of the inline helpers");

extern "C" int sdsm_neighbour_halfwidth(int max_d2, int d_row)
{
    return sdsm_neighbour_halfwidth_inline(max_d2, d_row);
}

extern "C" int64_t sdsm_neighbour_slot(uint64_t key, int64_t capacity)
{
    if (capacity < 1 || (capacity & (capacity - 1)) != 0) return -1;
    return (int64_t)sdsm_neighbour_slot_inline(key, (uint64_t)capacity);
}

// The class of a bit quad, as the tile kernel of the connected parts takes it (sdsm_parts.h: the same inline function).
extern "C" int sdsm_parts_quad(int32_t a, int32_t b, int32_t c, int32_t d, int32_t label)
{
    return sdsm_parts_quad_inline(a, b, c, d, label);
}
