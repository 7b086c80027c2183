// TEST INFRASTRUCTURE ONLY -- the pieces of the n-frame RGB search calls on the CPU wave emulator: rgb_sse_kernel with the
// launch and the arguments kernel_select.hpp gives it (and a short-run instantiation, so that the widening runs), the
// unfused launches over the same data, the probe sequence of launch_seq.hpp over n RGB frames behind the unit-step
// transform as search_impl runs them, the candidate-count function and the size walk of rate_search.hpp.
// Built by tests/test_rgb_search_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

// out[3 f + k] = the SSE of plane k of frame f: the inverse ICT of the float planes (plane 3 f + k at c + (3 f + k) * c_z
// bytes) against the input planes.  max_wgs > 0 caps the grid; short_run: the instantiation that widens after two tiles.
// Returns 1 when the fused kernel ran, 0 when select_rgb_sse refused (nothing is launched then, `out` untouched).
int emu_rgb_sse(const float *c, unsigned long long c_z, unsigned long long c_pitch, const uint8_t *r, const uint8_t *g, const uint8_t *b,
                unsigned long long in_z, unsigned long long in_pitch, int w, int h, int n, int off, unsigned long long *out, int max_wgs,
                int short_run, int fused)
{
    const RgbSseArgs s = rgb_sse_args(c, c_z, (size_t)c_pitch, r, g, b, in_z, (size_t)in_pitch, w, h, n, off, out);
    RgbSseLaunch l = select_rgb_sse(s, fused != 0);
    if (!l.kernel) return 0;
    if (max_wgs > 0 && l.wgs > (unsigned)max_wgs) l.wgs = (unsigned)max_wgs;
    if (short_run) l.kernel = rgb_sse_kernel<2 * kRgbSseTileLoads>;
    go(sse_zero_kernel, dim3(1), 64u, out, 3 * n);
    go(l.kernel, dim3(l.wgs), 256u, s);
    return 1;
}

// the unfused launches over the same data (row pitch aw on both sides): rgb_inverse_kernel into pix (3 P bytes a frame),
// frames_sse of every plane
int emu_rgb_sse_unfused(const float *c, unsigned long long c_z, const uint8_t *r, const uint8_t *g, const uint8_t *b, unsigned long long in_z,
                        int w, int h, int aw, int ah, int n, int off, uint8_t *pix, unsigned long long *out)
{
    const size_t P = (size_t)aw * ah;
    for (int f = 0; f < n; f++) {
        const char *c0 = (const char *)c + (size_t)(3 * f) * c_z;
        uint8_t *px = pix + (size_t)(3 * f) * P;
        if (rgb_inverse(go, true, c0, c0 + c_z, c0 + 2 * c_z, px, px + P, px + 2 * P, P / 4, off)) return -1;
        const uint8_t *in[3] = { r + f * in_z, g + f * in_z, b + f * in_z };
        for (int k = 0; k < 3; k++)
            if (frames_sse(go, px + (size_t)k * P, (size_t)aw, 0, in[k], (size_t)aw, 0, w, h, 1, out + 3 * f + k)) return -1;
    }
    return 0;
}

// A probe of n RGB frames (frame f's planes frame_stride bytes after r / g / b): the unit transform as rate_transform
// runs it, then quality_probe at j; out[0 .. 3 n).  Returns -1 on an error, else 1 when the fused tail ran, 0 for the
// unfused one.  The buffers are the driver's own.
int emu_rgb_probe(const uint8_t *r, const uint8_t *g, const uint8_t *b, unsigned long long frame_stride, int w, int h, int aw, int ah,
                  int wl, int n, int j, unsigned long long *out, int fused)
{
    const int nf = 3 * n;
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), unit_z = ((P + extra + 3) & ~(size_t)3) * 4;
    std::vector<float> unit_raw((size_t)nf * unit_z / 4 + 16), work_raw((size_t)nf * (P + extra) + 16), planes_raw((size_t)nf * P + 16);
    std::vector<int32_t> coef_raw((size_t)nf * P + 16);
    std::vector<uint8_t> pix_raw((size_t)nf * P + 64);
    auto al = [](void *p) { return (void *)(((uintptr_t)p + 63u) & ~(uintptr_t)63u); };
    void *unit = al(unit_raw.data());
    auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward_unit(src, u8in, unit, aw, ah, wl); };
    const bool aligned = ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b) | (n > 1 ? frame_stride : 0)) & 15u) == 0;
    if (rgb_forward_transform(go, true, aligned, plan_of, false, r, g, b, al(planes_raw.data()), P, 128, unit_z, nullptr, nullptr, (unsigned)n,
                              frame_stride)) return -1;
    QualityProbe p = { unit, (unsigned long long)unit_z, (int32_t *)al(coef_raw.data()), al(work_raw.data()), (uint8_t *)al(pix_raw.data()),
                       aw, ah, wl, w, h, 128, P, extra, nf, nullptr, (size_t)frame_stride, r, g, b };
    p.rgb_sse_fused = fused != 0;
    const int took = quality_probe_fuses(p) ? 1 : 0;
    return quality_probe(go, p, j, out) ? -1 : took;
}

int emu_rgb_search_candidates(int size_search, int n, int force_one) { return rgb_search_candidates(size_search != 0, n, force_one != 0); }

// The walk the size calls run (bisect_walk, largest passing index) with a table lookup as its measure.  Returns the
// result j, 0 when nothing fits, -1 for a range without a grid entry.  stats: { rounds, probes used, probes made }.
int emu_rgb_size_walk(const unsigned long long *size_by_j, unsigned long long limit, int j_min, int j_max, int K, int *stats)
{
    if (!rate_range_ok(j_min, j_max)) return -1;
    const std::vector<int> grid = rate_grid(j_min, j_max);
    if (grid.empty()) return -1;
    int made = 0;
    const BisectWalk w = bisect_walk(grid, (uint64_t)limit, K, Bisect::Largest, [&](int m, const int *js, uint64_t *v) {
        for (int i = 0; i < m; i++, made++) v[i] = (uint64_t)size_by_j[js[i]];
        return 0;
    });
    if (stats) { stats[0] = w.rounds; stats[1] = w.probes; stats[2] = made; }
    return w.result < 0 ? 0 : grid[(size_t)w.result];
}

}  // extern "C"
