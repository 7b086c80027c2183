// TEST INFRASTRUCTURE ONLY -- the window decode (picsong_decode_frame_window) on the CPU wave emulator: the decoder over
// the rectangle table of window_plan and the cone's synthesis (dwt_window_kernel), through the same plan functions
// (launch_plan.hpp, window_kernels.hpp), the same choice of kernel, grid and scratch (kernel_select.hpp) and the same
// kernel sources as cuda-image-and-video-codec_amd/csrc/picsong_hip.hip.
// Built by tests/test_window_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/kernel_select.hpp"

using namespace picsong;

extern "C" {

// window_plan: rects = 4 ints a rectangle (codeblock units, x0, y0, x1, y1), n[0] = rectangles, n[1] = codeblocks they
// list, n[2] = window_waves, n[3] = window_waves_cap (4-wave workgroups); returns the distinct codeblocks
int emu_window_plan(int aw, int ah, int wl, int lossy, int r, int x, int y, int w, int h, int *rects, int *n)
{
    const WindowPlan p = window_plan(aw, ah, wl, lossy != 0, r, x, y, w, h);
    for (int i = 0; i < p.n_rects; i++) {
        rects[4 * i] = p.cb[i].x0; rects[4 * i + 1] = p.cb[i].y0; rects[4 * i + 2] = p.cb[i].x1; rects[4 * i + 3] = p.cb[i].y1;
    }
    n[0] = p.n_rects; n[1] = p.n_cb_listed; n[2] = window_waves(p);
    n[3] = window_waves_cap(aw, ah, wl, lossy != 0, (aw / 64) * (ah / 64), 4);
    return p.n_cb;
}
int emu_window_ok(int paw, int pah, int x, int y, int w, int h) { return window_ok(paw, pah, x, y, w, h) ? 1 : 0; }

// One frame's window, as picsong_decode_frame_window runs it: the lengths and offsets of the whole stream, the decoder
// over the plan's rectangle table (k = 0 or -k > 0; from the stream itself, or through the staging when `staging` is
// set; 32-bit coefficients), the synthesis levels wl - 1 .. r over the cone, pixels into the window (row stride pitch).
// coef: the decoder's output array (AW * AH int32), filled by the caller.  Returns bit 3: the lengths were damaged.
int emu_decode_window(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, int lossy, float qs,
                      const int32_t *lut, const int *geo, float k, int n_tables, int staging, int r, int x, int y, int w,
                      int h, int32_t *coef, uint8_t *pixels, size_t pitch, int *flag)
{
    const int ncb = (aw / 64) * (ah / 64);
    const WindowPlan plan = window_plan(aw, ah, wl, lossy != 0, r, x, y, w, h);
    const size_t P = (size_t)aw * ah;
    const size_t extra = [&] { size_t e = 0; for (int l = 1; l < wl; l++) e += (size_t)(aw >> l) * (size_t)(ah >> l); return e; }();
    std::vector<float> work(P + extra, std::nanf(""));

    std::vector<int32_t> sizes(ncb), offsets(ncb), stage;
    int32_t total = 0;
    int bad = 0, res = 0;
    BpcArgs a = bpc_frame_args(aw, ah, wl, lut, lut_geo(geo), flag);
    a.sizes = sizes.data(); a.coeffs_out = coef;
    a.k = k; a.n_tables = n_tables;
    const unsigned waves = (unsigned)window_bpc_table(a, plan);
    if (staging) {
        stage.assign((size_t)ncb * 4096, 0);
        emu::launch(dim3((unsigned)((ncb + 255) / 256)), dim3(256), [&] { read_sizes_kernel(stream, ncb, sizes.data(), &bad); });
        emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_sizes_kernel(sizes.data(), ncb, offsets.data(), &total); });
        emu::launch(dim3((unsigned)ncb), dim3(256), [&] { unpack_kernel(stream, sizes.data(), offsets.data(), ncb, stage.data()); });
        a.staging = stage.data();
    } else {
        emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_stream_kernel(stream, ncb, sizes.data(), offsets.data(), &total, &bad, 0); });
        a.cw16 = stream; a.cw16_offsets = offsets.data(); a.cw16_total = &total; a.cw16_max = stream_shorts;
    }
    if (bad) res |= 8;
    // (32-bit coefficients: a window's synthesis reads no 16-bit ones)
    const BpcLaunch dec = select_decoder(false, k > 0.0f, k > 0.0f && bulk_compact(aw, ah, wl, a.g), !staging, false, waves);
    std::vector<uint32_t> ps(dec.scratch_dwords, 0xDEADBEEFu);
    a.plane_scratch = ps.data();
    emu::launch(dim3(dec.wgs), dim3(dec.threads), [&] { dec.kernel(a); });

    // ---- the cone's synthesis (run_window)
    std::vector<WinLaunch> syn = plan_window_synthesis(plan, coef, work.data(), P, aw, ah, qs, pixels, pitch, 128);
    for (const WinLaunch &f : syn) {
        const WinKernel kw = select_window(lossy != 0, f.u8);
        emu::launch(f.grid, dim3(256), [&] { kw(f.a); });
    }
    return res;
}

}  // extern "C"
