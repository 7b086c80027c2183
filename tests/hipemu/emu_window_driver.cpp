// TEST INFRASTRUCTURE ONLY -- the window decode (picsong_decode_frame_window, picsong_decode_frames_window) on the CPU wave
// emulator: the decoder over the rectangle table of window_plan and the cone's synthesis (dwt_window_kernel), through the
// library's own sequence (decode_frames, launch_seq.hpp) over a context of this file's making (emu_decode_ctx.hpp), with
// the plan functions (launch_plan.hpp, window_kernels.hpp), choice of kernel, grid and scratch (kernel_select.hpp) and
// kernel sources of cuda-image-and-video-codec_amd/csrc/picsong_hip.hip, run through the emulator's launcher.
// Built by tests/test_window_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include "emu_decode_ctx.hpp"

extern "C" {

int emu_window_launches(void) { return g_launches; }
void emu_window_reset(void) { g_launches = 0; }

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

// The windows of n frames, as picsong_decode_frames_window runs them (n = 1: picsong_decode_frame_window): the lengths and
// offsets of the whole streams, stream_shorts apart, the decoder over the plan's rectangle table (k = 0 or -k > 0; from
// the streams themselves, or through the staging when `staging` is set; 32-bit coefficients), the synthesis levels
// wl - 1 .. r over the cone, pixels into frame f's window at pixels + f * frame_stride (row stride pitch).
// coef: the decoder's output arrays (n x AW * AH int32), filled by the caller.  Returns bit 3: the lengths were damaged.
int emu_decode_window(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, int lossy, float qs,
                      const int32_t *lut, const int *geo, float k, int n_tables, int staging, int r, int x, int y, int w,
                      int h, int32_t *coef, uint8_t *pixels, size_t pitch, int *flag, int n, size_t frame_stride)
{
    const WindowPlan plan = window_plan(aw, ah, wl, lossy != 0, r, x, y, w, h);
    Ctx c(n, false, aw, ah, wl, lossy, qs, lut, nullptr, nullptr, geo, k, n_tables, flag, stream_shorts, staging != 0, coef);
    if (decode_frames(go, c.g, c.a, c.w, (unsigned)n, stream, stream_shorts, r, &plan, false, true, pixels, frame_stride, pitch)) return -1;
    return c.bad ? 8 : 0;
}

}  // extern "C"
