// TEST INFRASTRUCTURE ONLY -- the rate calls' pieces on the CPU wave emulator: the search (bisect_walk of
// rate_search.hpp, the very loop picsong_hip.hip's search_impl runs), the unquantised forward transform (plan_dwt_forward_unit through rate_transform's
// sequences: launch_fwd_plan, rgb_forward_transform, launch_seq.hpp) and quantise_kernel with the launch and the
// arguments kernel_select.hpp gives it.
// Built by tests/test_rate_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

float emu_rate_q(int j) { return rate_q(j); }
int emu_rate_header_exact(int j) { return rate_header_exact(j) ? 1 : 0; }

// G' into out (capacity cap); returns its length, -1 for a bad range
int emu_rate_grid(int j_min, int j_max, int *out, int cap)
{
    if (!rate_range_ok(j_min, j_max)) return -1;
    const std::vector<int> g = rate_grid(j_min, j_max);
    for (size_t i = 0; i < g.size() && (int)i < cap; i++) out[i] = g[i];
    return (int)g.size();
}

// The walk the rate calls run (bisect_walk, rate_search.hpp) with a table lookup as its measure: a synthetic size
// function size_by_j[0 .. 16383] (the tests' tables and targets are positive, as the coder's totals are: the library's cast).
// Returns the result j, 0 when nothing fits, -1 for a range without a grid entry.  stats: { rounds, probes used, probes
// made }; probed (capacity 64): the j of every probe made, round by round.
int emu_rate_search(const long long *size_by_j, long long target, int j_min, int j_max, int K, int *stats, int *probed)
{
    if (!rate_range_ok(j_min, j_max)) return -1;
    const std::vector<int> grid = rate_grid(j_min, j_max);
    if (grid.empty()) return -1;
    int made = 0;
    const BisectWalk w = bisect_walk(grid, (uint64_t)target, K, Bisect::Largest, [&](int m, const int *js, uint64_t *v) {
        for (int i = 0; i < m; i++, made++) {
            v[i] = (uint64_t)size_by_j[js[i]];
            if (probed && made < 64) probed[made] = js[i];
        }
        return 0;
    });
    if (stats) { stats[0] = w.rounds; stats[1] = w.probes; stats[2] = made; }
    return w.result < 0 ? 0 : grid[(size_t)w.result];
}

// the unquantised transform of `frames` frames (u8 with the level shift fused, or float), frame z at in + z * in_z bytes,
// into the float work buffers out + z * out_z bytes; returns 1 when levels 0 and 1 went through the fused head
int emu_rate_unit_forward(const void *in, int u8in, unsigned long long in_z, void *out, unsigned long long out_z, int aw,
                          int ah, int wl, int frames)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward_unit(in, u8in != 0, out, aw, ah, wl);
    plan_frame_strides(plan, in_z, out_z);
    bool fused01 = false;
    launch_fwd_plan(go, true, plan, (unsigned)frames, &fused01);
    return fused01 ? 1 : 0;
}

// an RGB frame's three components, the ICT in the fused head's load stage (rate_transform's first form); 0: the form
// does not apply to the geometry
int emu_rate_unit_forward_rgb(const uint8_t *r, const uint8_t *g, const uint8_t *b, void *out, unsigned long long out_z,
                              int aw, int ah, int wl)
{
    const size_t P = (size_t)aw * ah;
    std::vector<float> planes(3 * P);
    auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward_unit(src, u8in, out, aw, ah, wl); };
    bool fused = false;
    rgb_forward_transform(go, true, true, plan_of, false, r, g, b, planes.data(), P, 128, out_z, nullptr, &fused);
    return fused ? 1 : 0;
}

// quantise_kernel over n float arrays for the K candidates js (candidate c as int16 where c16[c]); max_wgs > 0 caps the
// grid (a workgroup then takes several rows)
void emu_rate_quantise(const void *src, unsigned long long src_z, void *dst, unsigned long long dst_z, int aw, int ah, int wl,
                       int n, int K, const int *js, const int *c16, int max_wgs)
{
    bool forms[kQuantMaxK] = { false, false, false };
    for (int c = 0; c < K; c++) forms[c] = c16[c] != 0;
    const QuantArgs a = quantise_args(src, src_z, dst, dst_z, aw, ah, wl, n, K, js, forms);
    QuantLaunch l = select_quantise(K, n, ah);
    if (max_wgs > 0 && l.wgs > (unsigned)max_wgs) l.wgs = (unsigned)max_wgs;
    go(l.kernel, dim3(l.wgs), 256u, a);
}

int emu_rate_coef16_ok(int wl, int j, int in_max, int aw, int ah)
{
    return coef16_ok(true, wl, rate_q(j), in_max) && dwt_c16_geometry_ok(aw, ah, wl) ? 1 : 0;
}

}  // extern "C"
