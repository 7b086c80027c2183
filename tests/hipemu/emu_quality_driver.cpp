// TEST INFRASTRUCTURE ONLY -- the quality calls' pieces on the CPU wave emulator: sse_kernel with the launch and the
// arguments kernel_select.hpp gives it, the search (bisect_walk of rate_search.hpp, the very loop picsong_hip.hip's
// search_impl runs), quantise_kernel's int32 form, and the probe sequence of launch_seq.hpp (quality_probe) behind the
// unit-step transform, as search_impl runs them.
// Built by tests/test_quality_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

// out[0 .. n) = the SSE of n pairs of arrays; max_wgs = 0: the frames_sse sequence as the library runs it; > 0: the same
// two launches with the grid capped (a workgroup then takes many tiles, of several frames).  Returns 1 for the vector form.
int emu_sse(const uint8_t *a, unsigned long long a_pitch, unsigned long long a_z, const uint8_t *b, unsigned long long b_pitch,
            unsigned long long b_z, int w, int h, int n, unsigned long long *out, int max_wgs)
{
    const SseArgs s = sse_args(a, (size_t)a_pitch, a_z, b, (size_t)b_pitch, b_z, w, h, n, out);
    SseLaunch l = select_sse(s);
    if (max_wgs <= 0) {
        frames_sse(go, a, (size_t)a_pitch, a_z, b, (size_t)b_pitch, b_z, w, h, n, out);
    } else {
        if (l.wgs > (unsigned)max_wgs) l.wgs = (unsigned)max_wgs;
        go(sse_zero_kernel, dim3(1), 64u, out, n);
        go(l.kernel, dim3(l.wgs), 256u, s);
    }
    return l.kernel == (SseKernel)sse_kernel<true> ? 1 : 0;
}

// The walk the quality calls run (bisect_walk, rate_search.hpp) with a table lookup as its measure: a synthetic
// distortion sse_by_j[0 .. 16383].  Returns the result j, 0 when nothing meets the limit, -1 for a range without a grid
// entry.  stats: { rounds, probes used, probes made }; probed (capacity 64): the j of every probe made, round by round.
int emu_quality_search(const unsigned long long *sse_by_j, unsigned long long limit, int j_min, int j_max, int K, int *stats,
                       int *probed)
{
    if (!rate_range_ok(j_min, j_max)) return -1;
    const std::vector<int> grid = rate_grid(j_min, j_max);
    if (grid.empty()) return -1;
    int made = 0;
    const BisectWalk w = bisect_walk(grid, (uint64_t)limit, K, Bisect::Smallest, [&](int m, const int *js, uint64_t *v) {
        for (int i = 0; i < m; i++, made++) {
            v[i] = (uint64_t)sse_by_j[js[i]];
            if (probed && made < 64) probed[made] = js[i];
        }
        return 0;
    });
    if (stats) { stats[0] = w.rounds; stats[1] = w.probes; stats[2] = made; }
    return w.result < 0 ? 0 : grid[(size_t)w.result];
}

// the unit-step transform of `frames` u8 frames (in_z bytes apart) into float work buffers out_z bytes apart
void emu_quality_unit_forward(const uint8_t *in, unsigned long long in_z, void *out, unsigned long long out_z, int aw, int ah,
                              int wl, int frames)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward_unit(in, true, out, aw, ah, wl);
    plan_frame_strides(plan, in_z, out_z);
    launch_fwd_plan(go, true, plan, (unsigned)frames);
}

// quantise_kernel's int32 form over n float arrays at q(j), array f at dst + f * dst_z
void emu_quality_quantise_i32(const void *src, unsigned long long src_z, void *dst, unsigned long long dst_z, int aw, int ah,
                              int wl, int n, int j)
{
    const bool forms[kQuantMaxK] = { false, false, false };
    const QuantArgs a = quantise_args(src, src_z, dst, dst_z, aw, ah, wl, n, 1, &j, forms);
    const QuantLaunch l = select_quantise(1, n, ah, true);
    go(l.kernel, dim3(l.wgs), 256u, a);
}

// A probe of nf grey frames (frame_stride bytes apart) or, with g and b, of an RGB frame (`frames` = R): the unit
// transform as rate_transform runs it, then quality_probe at j; out[0 .. nf).  The buffers are the driver's own.
int emu_quality_probe(const uint8_t *frames, unsigned long long frame_stride, const uint8_t *g, const uint8_t *b, int w, int h,
                      int aw, int ah, int wl, int nf, int j, unsigned long long *out)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), unit_z = ((P + extra + 3) & ~(size_t)3) * 4;
    std::vector<float> unit_raw((size_t)nf * unit_z / 4 + 16), work_raw((size_t)nf * (P + extra) + 16), planes_raw(3 * P + 16);
    std::vector<int32_t> coef_raw((size_t)nf * P + 16);
    std::vector<uint8_t> pix_raw((size_t)nf * P + 64);
    auto al = [](void *p) { return (void *)(((uintptr_t)p + 63u) & ~(uintptr_t)63u); };
    void *unit = al(unit_raw.data());
    const bool rgb = g != nullptr;
    if (rgb) {
        auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward_unit(src, u8in, unit, aw, ah, wl); };
        const bool aligned = ((((uintptr_t)frames) | ((uintptr_t)g) | ((uintptr_t)b)) & 15u) == 0;
        if (rgb_forward_transform(go, true, aligned, plan_of, false, frames, g, b, al(planes_raw.data()), P, 128, unit_z)) return -1;
    } else {
        emu_quality_unit_forward(frames, frame_stride, unit, unit_z, aw, ah, wl, nf);
    }
    const QualityProbe p = { unit, (unsigned long long)unit_z, (int32_t *)al(coef_raw.data()), al(work_raw.data()),
                             (uint8_t *)al(pix_raw.data()), aw, ah, wl, w, h, 128, P, extra, nf,
                             rgb ? nullptr : frames, (size_t)frame_stride, rgb ? frames : nullptr, g, b };
    return quality_probe(go, p, j, out);
}

}  // extern "C"
