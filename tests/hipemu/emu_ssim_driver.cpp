// TEST INFRASTRUCTURE ONLY -- the SSIM calls' pieces on the CPU wave emulator: ssim_kernel with the launch and the
// arguments kernel_select.hpp gives it (select_ssim), the frames_dssim sequence of launch_seq.hpp, the probe sequence
// (quality_probe with QualityProbe::ssim) behind the unit-step transform, and the search (bisect_walk of rate_search.hpp,
// the very loop picsong_hip.hip's search_impl runs) over such probes.
// Built by tests/test_ssim_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

// out[0 .. n) = the DSSIM sums of n pairs of arrays; max_wgs = 0: the frames_dssim sequence as the library runs it; > 0:
// the same two launches with the grid capped (a workgroup then takes many tiles, of several frames).  Returns 1 for the
// dword form, 0 for the per-byte one.
int emu_dssim(const uint8_t *a, unsigned long long a_pitch, unsigned long long a_z, const uint8_t *b, unsigned long long b_pitch,
              unsigned long long b_z, int w, int h, int n, unsigned long long *out, int max_wgs)
{
    const SseArgs s = sse_args(a, (size_t)a_pitch, a_z, b, (size_t)b_pitch, b_z, w, h, n, out);
    SseLaunch l = select_ssim(s);
    if (max_wgs <= 0) {
        frames_dssim(go, a, (size_t)a_pitch, a_z, b, (size_t)b_pitch, b_z, w, h, n, out);
    } else {
        if (l.wgs > (unsigned)max_wgs) l.wgs = (unsigned)max_wgs;
        go(sse_zero_kernel, dim3(1), 64u, out, n);
        go(l.kernel, dim3(l.wgs), 256u, s);
    }
    return l.kernel == (SseKernel)ssim_kernel<true> ? 1 : 0;
}

// the kernel's shape, for the tests' own arithmetic: { window columns a wave strip, window rows a band }
void emu_ssim_shape(int *shape)
{
    shape[0] = kSsimStripWindows;
    shape[1] = kSsimBandWindows;
}

struct ProbeBuffers {
    std::vector<float> unit_raw, work_raw, planes_raw;
    std::vector<int32_t> coef_raw;
    std::vector<uint8_t> pix_raw;
    QualityProbe p;
};
static void *al(void *p) { return (void *)(((uintptr_t)p + 63u) & ~(uintptr_t)63u); }

// the unit-step transform of nf grey frames (frame_stride bytes apart) or, with g and b, of an RGB frame (`frames` = R),
// as rate_transform runs it, and the probe over the driver's own buffers
static int make_probe(ProbeBuffers &B, const uint8_t *frames, unsigned long long frame_stride, const uint8_t *g, const uint8_t *b,
                      int w, int h, int aw, int ah, int wl, int nf)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), unit_z = ((P + extra + 3) & ~(size_t)3) * 4;
    B.unit_raw.resize((size_t)nf * unit_z / 4 + 16); B.work_raw.resize((size_t)nf * (P + extra) + 16); B.planes_raw.resize(3 * P + 16);
    B.coef_raw.resize((size_t)nf * P + 16);
    B.pix_raw.resize((size_t)nf * P + 64);
    void *unit = al(B.unit_raw.data());
    const bool rgb = g != nullptr;
    if (rgb) {
        auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward_unit(src, u8in, unit, aw, ah, wl); };
        const bool aligned = ((((uintptr_t)frames) | ((uintptr_t)g) | ((uintptr_t)b)) & 15u) == 0;
        if (rgb_forward_transform(go, true, aligned, plan_of, false, frames, g, b, al(B.planes_raw.data()), P, 128, unit_z)) return -1;
    } else {
        std::vector<FwdLaunch> plan = plan_dwt_forward_unit(frames, true, unit, aw, ah, wl);
        plan_frame_strides(plan, frame_stride, unit_z);
        launch_fwd_plan(go, true, plan, (unsigned)nf);
    }
    B.p = QualityProbe{ unit, (unsigned long long)unit_z, (int32_t *)al(B.coef_raw.data()), al(B.work_raw.data()),
                        (uint8_t *)al(B.pix_raw.data()), aw, ah, wl, w, h, 128, P, extra, nf,
                        rgb ? nullptr : frames, (size_t)frame_stride, rgb ? frames : nullptr, g, b, true, true };
    return 0;
}

// One SSIM probe at each of js[0 .. nj): quantise, dividing synthesis (RGB: inverse ICT into pixels), ssim_kernel against
// the input; out[i * nf .. (i + 1) * nf) = the DSSIM sums at js[i].
int emu_ssim_probe(const uint8_t *frames, unsigned long long frame_stride, const uint8_t *g, const uint8_t *b, int w, int h,
                   int aw, int ah, int wl, int nf, const int *js, int nj, unsigned long long *out)
{
    ProbeBuffers B;
    if (make_probe(B, frames, frame_stride, g, b, w, h, aw, ah, wl, nf)) return -1;
    for (int i = 0; i < nj; i++)
        if (int rc = quality_probe(go, B.p, js[i], out + (size_t)i * nf)) return rc;
    return 0;
}

// The search the SSIM calls run: bisect_walk (K candidates a round, the smallest passing index) with such probes as its
// measure.  Returns the result j, 0 when nothing meets the limit, -1 for a range without a grid entry; result_dssim[nf]:
// the result's per-array sums; stats: { rounds, probes used, probes made }; probed (capacity 64): the j of every probe made.
int emu_ssim_search(const uint8_t *frames, unsigned long long frame_stride, const uint8_t *g, const uint8_t *b, int w, int h,
                    int aw, int ah, int wl, int nf, unsigned long long limit, int j_min, int j_max, int K,
                    unsigned long long *result_dssim, int *stats, int *probed)
{
    if (!rate_range_ok(j_min, j_max)) return -1;
    const std::vector<int> grid = rate_grid(j_min, j_max);
    if (grid.empty()) return -1;
    ProbeBuffers B;
    if (make_probe(B, frames, frame_stride, g, b, w, h, aw, ah, wl, nf)) return -1;
    int made = 0;
    std::vector<int> seen_j;
    std::vector<unsigned long long> seen, sums((size_t)nf);
    const BisectWalk wk = bisect_walk(grid, (uint64_t)limit, K, Bisect::Smallest, [&](int m, const int *js, uint64_t *v) {
        for (int i = 0; i < m; i++, made++) {
            if (int rc = quality_probe(go, B.p, js[i], sums.data())) return rc;
            seen_j.push_back(js[i]);
            for (int f = 0; f < nf; f++) { v[i] += sums[(size_t)f]; seen.push_back(sums[(size_t)f]); }
            if (probed && made < 64) probed[made] = js[i];
        }
        return 0;
    });
    if (stats) { stats[0] = wk.rounds; stats[1] = wk.probes; stats[2] = made; }
    if (wk.rc) return -2;
    if (wk.result < 0) return 0;
    const int j = grid[(size_t)wk.result];
    for (size_t i = 0; i < seen_j.size(); i++)
        if (seen_j[i] == j) for (int f = 0; f < nf; f++) result_dssim[f] = seen[i * (size_t)nf + (size_t)f];
    return j;
}

}  // extern "C"
