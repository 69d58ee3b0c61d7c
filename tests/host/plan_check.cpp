// Stand-alone check of the plan unit (superdsm_amd/csrc/sdsm_plan.hip, linked alone: no device, no HIP runtime call) for a build with
// the address and undefined-behaviour sanitizers on the host side only (tests/test_plan_host_cpu.py).  usage: plan_check CASES OUTDIR.  CASES: the plans of
// superdsm_amd.testing.PLAN_LAYOUT_CASES as that module writes them (plan_cases_text).  Per case the program walks the three scheduling modes,
// calls every query of the plan, and writes for each recorded mode KEY = name.mode<m>: KEY.params, KEY.cand (sdsm_plan_image), KEY.lists (14
// span words, then `order`) and KEY.sizes (int64: workspace bytes, mask bytes, total pixels, xi count, the 16 values of sdsm_plan_layout).  Then
// it makes the calls the API rejects.  Exit status 0 and nothing on stderr: every call answered as documented.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/sdsm.h"

static const size_t PARAMS_BYTES = 856, CAND_BYTES = 112;     // sizeof(BatchParams), sizeof(CandDesc)
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "plan_check: line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

struct Case {
    std::string name;
    std::vector<int> modes;
    std::vector<int32_t> H, W, n_atoms, offsets, labels, image_of;
    std::vector<std::vector<int32_t>> stats;
    sdsm_dsm_config cfg;
    int n;
    sdsm_plan *create() const
    {
        std::vector<const int32_t *> tables;
        for (const auto &s : stats) tables.push_back(s.data());
        if (tables.size() == 1) return sdsm_plan_create(H[0], W[0], n_atoms[0], tables[0], &cfg, n, offsets.data(), labels.data());
        return sdsm_plan_create_multi((int)tables.size(), H.data(), W.data(), n_atoms.data(), tables.data(), &cfg, n, offsets.data(), labels.data(), image_of.data());
    }
};

static std::vector<Case> read_cases(const char *path)
{
    std::ifstream in(path);
    std::string tok;
    auto word = [&] { in >> tok; if (!in) { fprintf(stderr, "plan_check: %s ends early\n", path); exit(2); } return tok; };
    auto num = [&] { return strtod(word().c_str(), nullptr); };          // (strtod reads "inf")
    auto ints = [&](size_t count) { std::vector<int32_t> v(count); for (auto &x : v) x = (int32_t)num(); return v; };
    std::vector<Case> cases((size_t)num());
    for (Case &c : cases) {
        c.name = word();
        for (int32_t m : ints((size_t)num())) c.modes.push_back(m);
        const size_t n_images = (size_t)num();
        c.H = ints(n_images); c.W = ints(n_images); c.n_atoms = ints(n_images);
        for (size_t im = 0; im < n_images; im++) c.stats.push_back(ints((size_t)(c.n_atoms[im] + 1) * SDSM_ATOM_STATS_STRIDE));
        c.cfg.scale = num(); c.cfg.epsilon = num(); c.cfg.alpha = num(); c.cfg.smooth_amount = num(); c.cfg.gaussian_shape_multiplier = num(); c.cfg.background_margin = num();
        c.cfg.smooth_subsample = (int)num(); c.cfg.init_elliptical = (int)num(); c.cfg.max_iters = (int)num(); c.cfg.flags = (int)num();
        c.n = (int)num();
        c.offsets = ints((size_t)c.n + 1);
        c.labels = ints((size_t)c.offsets[c.n]);
        c.image_of = ints((size_t)c.n);
    }
    return cases;
}

static void write_file(const std::string &path, const void *data, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes || fclose(f) != 0) { fprintf(stderr, "plan_check: cannot write %s\n", path.c_str()); exit(2); }
}

// Every query of a plan in its current mode; the files of the mode if `key` is not empty.
static void walk(const Case &c, sdsm_plan *p, const std::string &key)
{
    const size_t n = (size_t)c.n, n1 = n ? n : 1;
    int64_t sizes[20] = {(int64_t)sdsm_plan_workspace_bytes(p), (int64_t)sdsm_plan_mask_bytes(p), sdsm_plan_total_pixels(p), sdsm_plan_xi_count(p)};
    CHECK(sizes[0] > 0 && sizes[0] % 256 == 0 && sizes[1] >= 4 && sizes[3] >= 1);
    CHECK(sdsm_plan_layout(p, sizes + 4) == SDSM_OK);
    CHECK(sdsm_plan_eval_param_count(p) == 6 * (int64_t)n + sizes[3] && sdsm_plan_eval_out_count(p) == 29 * (int64_t)n + sizes[3]);
    std::vector<int32_t> info(4 * n1), npx(n1), g(n1), r(n1), cls(n1), status(n1, 0), M(n1), env(n1);
    std::vector<int64_t> moff(n1), xoff(n1);
    CHECK(sdsm_plan_describe(p, info.data(), moff.data(), npx.data()) == SDSM_OK);
    CHECK(sdsm_plan_describe(p, nullptr, nullptr, nullptr) == SDSM_OK && sdsm_plan_describe(p, info.data(), nullptr, nullptr) == SDSM_OK);
    CHECK(sdsm_plan_describe(p, nullptr, moff.data(), nullptr) == SDSM_OK && sdsm_plan_describe(p, nullptr, nullptr, npx.data()) == SDSM_OK);
    CHECK(sdsm_plan_schedule(p, g.data(), r.data()) == SDSM_OK && sdsm_plan_schedule(p, nullptr, r.data()) == SDSM_OK && sdsm_plan_schedule(p, g.data(), nullptr) == SDSM_OK);
    CHECK(sdsm_plan_schedule(p, nullptr, nullptr) == SDSM_OK);
    CHECK(sdsm_plan_xi_offsets(p, xoff.data()) == SDSM_OK);
    int64_t pixels = 0;
    for (size_t i = 0; i < n; i++) pixels += npx[i];
    CHECK(pixels == sizes[2]);
    // the solve classes for what a setup kernel might report: small, mid-size and oversized systems, and a candidate without a solve
    for (size_t i = 0; i < n; i++) { M[i] = (int32_t)(i % 4 == 3 ? 3000 : 40 * (i % 4) * (i % 7)); env[i] = M[i] * (M[i] + 1) / 2 % 20000; status[i] = i % 11 == 10 ? 2 : 0; }
    CHECK(sdsm_plan_solve_classes(p, status.data(), M.data(), env.data(), cls.data()) == SDSM_OK);
    for (size_t i = 0; i < n; i++) CHECK(cls[i] >= -1 && cls[i] <= 7 && (cls[i] == -1) == (status[i] != 0));
    CHECK(sdsm_set_light_envelope_limit(5000) == SDSM_OK && sdsm_plan_solve_classes(p, status.data(), M.data(), env.data(), cls.data()) == SDSM_OK);
    CHECK(sdsm_set_light_envelope_limit(-1) == SDSM_OK);
    int32_t spans[14];
    CHECK(sdsm_plan_lists(p, spans, nullptr) == SDSM_OK);
    size_t entries = 0;
    for (int l = 0; l < 7; l++) { CHECK(spans[2 * l] == (int32_t)entries && spans[2 * l + 1] >= 0); entries += (size_t)spans[2 * l + 1]; }
    std::vector<int32_t> lists(14 + entries);
    CHECK(sdsm_plan_lists(p, lists.data(), lists.data() + 14) == SDSM_OK && memcmp(spans, lists.data(), sizeof(spans)) == 0);
    CHECK((size_t)spans[1] == n);
    std::vector<uint8_t> params(PARAMS_BYTES), cand(CAND_BYTES * n1);
    CHECK(sdsm_plan_image(p, params.data(), PARAMS_BYTES, cand.data(), CAND_BYTES * n) == SDSM_OK);
    CHECK(sdsm_plan_image(p, params.data(), PARAMS_BYTES - 1, cand.data(), CAND_BYTES * n) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_image(p, params.data(), PARAMS_BYTES, cand.data(), CAND_BYTES * n + 1) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_image(p, nullptr, PARAMS_BYTES, cand.data(), CAND_BYTES * n) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_set_start(p, nullptr) == SDSM_OK);
    double x0 = 0;
    CHECK(sdsm_plan_set_start(p, &x0) == (c.cfg.init_elliptical ? SDSM_ERR_ARGUMENT : SDSM_OK) && sdsm_plan_set_start(p, nullptr) == SDSM_OK);
    if (key.empty()) return;
    write_file(key + ".params", params.data(), PARAMS_BYTES);
    write_file(key + ".cand", cand.data(), CAND_BYTES * n);
    write_file(key + ".lists", lists.data(), 4 * lists.size());
    write_file(key + ".sizes", sizes, sizeof(sizes));
}

// The calls the API documents as rejected: each returns its error (or no plan) and leaves a message.
static void rejected(const Case &c)
{
    std::vector<const int32_t *> tables;
    for (const auto &s : c.stats) tables.push_back(s.data());
    const int32_t *H = c.H.data(), *W = c.W.data(), *na = c.n_atoms.data(), *off = c.offsets.data(), *lab = c.labels.data(), *im = c.image_of.data();
    const int ni = (int)tables.size();
    auto none = [&](sdsm_plan *p) { const bool ok = p == nullptr && strlen(sdsm_last_error()) > 0; if (p) sdsm_plan_destroy(p); return ok; };
    CHECK(none(sdsm_plan_create_multi(0, H, W, na, tables.data(), &c.cfg, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(17, H, W, na, tables.data(), &c.cfg, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, nullptr, W, na, tables.data(), &c.cfg, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, nullptr, na, tables.data(), &c.cfg, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, nullptr, tables.data(), &c.cfg, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, nullptr, &c.cfg, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), nullptr, c.n, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &c.cfg, -1, off, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &c.cfg, c.n, nullptr, lab, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &c.cfg, c.n, off, nullptr, im)));
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &c.cfg, c.n, off, lab, nullptr)));      // several images need image_of
    std::vector<const int32_t *> hole = tables;
    hole[1] = nullptr;
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, hole.data(), &c.cfg, c.n, off, lab, im)));
    std::vector<int32_t> one = c.H;
    one[1] = 1;
    CHECK(none(sdsm_plan_create_multi(ni, one.data(), W, na, tables.data(), &c.cfg, c.n, off, lab, im)));
    for (int32_t bad : {-1, ni}) {
        std::vector<int32_t> of = c.image_of;
        of.back() = bad;
        CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &c.cfg, c.n, off, lab, of.data())) && strstr(sdsm_last_error(), "image index out of range"));
    }
    sdsm_dsm_config cfg = c.cfg;
    cfg.gaussian_shape_multiplier = 1.95;                      // round(1 + 4 * 4 * 1.95) = 32: an even PSF
    CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &cfg, c.n, off, lab, im)) && strstr(sdsm_last_error(), "must be odd"));
    for (int bad = 0; bad < 5; bad++) {
        cfg = c.cfg;
        if (bad == 0) cfg.epsilon = 0; else if (bad == 1) cfg.alpha = -1; else if (bad == 2) cfg.scale = 0; else if (bad == 3) cfg.smooth_subsample = 0; else cfg.smooth_amount = 0;
        CHECK(none(sdsm_plan_create_multi(ni, H, W, na, tables.data(), &cfg, c.n, off, lab, im)));
    }
    // a null plan: the size queries answer 0, the others are errors
    CHECK(sdsm_plan_workspace_bytes(nullptr) == 0 && sdsm_plan_mask_bytes(nullptr) == 0 && sdsm_plan_total_pixels(nullptr) == 0 && sdsm_plan_xi_count(nullptr) == 0);
    CHECK(sdsm_plan_eval_param_count(nullptr) == 0 && sdsm_plan_eval_out_count(nullptr) == 0);
    int32_t w32[16] = {0};
    int64_t w64[16] = {0};
    uint8_t blob[PARAMS_BYTES];
    CHECK(sdsm_plan_describe(nullptr, w32, w64, w32) == SDSM_ERR_ARGUMENT && sdsm_plan_schedule(nullptr, w32, w32) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_lists(nullptr, w32, nullptr) == SDSM_ERR_ARGUMENT && sdsm_plan_xi_offsets(nullptr, w64) == SDSM_ERR_ARGUMENT && sdsm_plan_layout(nullptr, w64) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_solve_classes(nullptr, w32, w32, w32, w32) == SDSM_ERR_ARGUMENT && sdsm_plan_image(nullptr, blob, PARAMS_BYTES, blob, 0) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_set_latency_mode(nullptr, 0) == SDSM_ERR_ARGUMENT && sdsm_plan_set_start(nullptr, nullptr) == SDSM_ERR_ARGUMENT);
    sdsm_plan_destroy(nullptr);
    sdsm_plan *p = c.create();
    CHECK(p != nullptr);
    if (!p) return;
    CHECK(sdsm_plan_lists(p, nullptr, nullptr) == SDSM_ERR_ARGUMENT && sdsm_plan_xi_offsets(p, nullptr) == SDSM_ERR_ARGUMENT && sdsm_plan_layout(p, nullptr) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_solve_classes(p, nullptr, w32, w32, w32) == SDSM_ERR_ARGUMENT && sdsm_plan_solve_classes(p, w32, w32, w32, nullptr) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_image(p, blob, PARAMS_BYTES, nullptr, CAND_BYTES * (size_t)c.n) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_plan_set_latency_mode(p, -1) == SDSM_ERR_ARGUMENT && sdsm_plan_set_latency_mode(p, 3) == SDSM_ERR_ARGUMENT);
    sdsm_plan_destroy(p);
    // the process-wide settings and the PSF
    CHECK(sdsm_set_light_envelope_limit(12401) == SDSM_ERR_ARGUMENT && sdsm_set_solver_diagnostics(2) == SDSM_ERR_ARGUMENT);
    CHECK(sdsm_set_solver_diagnostics(1) == SDSM_OK && sdsm_set_solver_diagnostics(0) == SDSM_OK && sdsm_set_group_timeout_us(10.0) == SDSM_OK && sdsm_set_group_timeout_us(0.0) == SDSM_OK);
    CHECK(sdsm_set_debug_buffer(nullptr) == SDSM_OK && sdsm_version() == SDSM_VERSION);
    CHECK(sdsm_psf(0.0, 2.0, nullptr) == SDSM_ERR_ARGUMENT && sdsm_psf(4.0, 2.0, nullptr) == 33);
    std::vector<float> psf(33 * 33);
    CHECK(sdsm_psf(4.0, 2.0, psf.data()) == 33 && psf[16 * 33 + 16] > psf[0] && psf[0] > 0);
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: plan_check CASES OUTDIR\n"); return 2; }
    const std::vector<Case> cases = read_cases(argv[1]);
    const Case *several = nullptr;
    for (const Case &c : cases) {
        sdsm_plan *p = c.create();
        CHECK(p != nullptr);
        if (!p) { fprintf(stderr, "plan_check: %s: %s\n", c.name.c_str(), sdsm_last_error()); continue; }
        for (int mode = 0; mode < 3; mode++) {
            CHECK(sdsm_plan_set_latency_mode(p, mode) == SDSM_OK);
            bool recorded = false;
            for (int m : c.modes) recorded = recorded || m == mode;
            walk(c, p, recorded ? std::string(argv[2]) + "/" + c.name + ".mode" + std::to_string(mode) : std::string());
        }
        sdsm_plan_destroy(p);
        if (c.stats.size() > 1 && c.n > 0) several = &c;
    }
    CHECK(several != nullptr);
    if (several) rejected(*several);
    return failures ? 1 : 0;
}
