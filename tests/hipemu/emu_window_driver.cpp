// TEST INFRASTRUCTURE ONLY -- the window decode (picsong_decode_frame_window) on the CPU wave emulator: the decoder over
// the rectangle table of window_plan and the cone's synthesis (dwt_window_kernel), through the same launch sequences
// (launch_seq.hpp: stream_intake, launch_decoder, run_window), plan functions (launch_plan.hpp, window_kernels.hpp),
// choice of kernel, grid and scratch (kernel_select.hpp) and kernel sources as
// cuda-image-and-video-codec_amd/csrc/picsong_hip.hip, run through the emulator's launcher.
// Built by tests/test_window_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

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
    std::vector<float> work(P + dwt_extra(aw, ah, wl), std::nanf(""));
    std::vector<int32_t> sizes(ncb), offsets(ncb), stage(staging ? (size_t)ncb * 4096 : 0, 0);
    int32_t total = 0;
    int bad = 0;
    BpcArgs a = bpc_frame_args(aw, ah, wl, lut, lut_geo(geo), flag);
    a.k = k; a.n_tables = n_tables;
    const unsigned waves = (unsigned)window_bpc_table(a, plan);
    std::vector<uint32_t> ps(decoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    const Workspace ws = { work.data(), stage.data(), sizes.data(), offsets.data(), &total, ps.data(), coef };
    stream_intake(go, stream, 1u, 0, !staging, ncb, P, ws, &bad);
    // (32-bit coefficients: a window's synthesis reads no 16-bit ones)
    launch_decoder(go, a, false, waves, k > 0.0f && bulk_compact(aw, ah, wl, a.g), ws, staging ? nullptr : stream, 0, stream_shorts, false);
    run_window(go, lossy != 0, plan, coef, work.data(), P, aw, ah, qs, 128, 1u, 0, 0, pixels, pitch, 0);
    return bad ? 8 : 0;
}

}  // extern "C"
