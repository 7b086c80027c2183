// TEST INFRASTRUCTURE ONLY -- the n-frame RGB proxy calls (picsong_decode_rgb_frames_reduced / _window,
// picsong_decode_rgb_images_reduced / _window) on the CPU wave emulator: their argument checks (kernel_select.hpp) and the
// launch sequences the library runs (decode_rgb_frames and decode_rgb_images_reduced, launch_seq.hpp), through a launcher
// that counts its launches.  What a context keeps -- the buffers (poisoned), the tables, the switches -- is
// emu_decode_ctx.hpp's.
// Built by tests/test_rgb_proxy_emulated.py with the flags of tests/hipemu/Makefile.
#include "emu_decode_ctx.hpp"

static int say(const char *why, char *msg, int cap)
{
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

extern "C" {

int emu_rgbp_launches(void) { return g_launches; }
void emu_rgbp_reset(void) { g_launches = 0; }

// 1 and the reason in msg when the calls refuse these arguments, else 0
int emu_rgbp_reduced_refusal(int ctx_rgb, int cp, int same_geometry, int n, const void *r, const void *g, const void *b, const void *streams,
                             unsigned long long frame_stride, unsigned long long stream_stride, int aw, int ah, int wl, int reduce, char *msg,
                             int cap)
{
    return say(rgb_frames_reduced_refusal(ctx_rgb != 0, cp, same_geometry != 0, n, r, g, b, streams, (size_t)frame_stride, (size_t)stream_stride,
                                          max_stream_shorts(aw, ah), aw, ah, wl, reduce), msg, cap);
}
int emu_rgbp_window_refusal(int ctx_rgb, int cp, int same_geometry, int n, const void *r, const void *g, const void *b, const void *streams,
                            unsigned long long pitch, unsigned long long frame_stride, unsigned long long stream_stride, int aw, int ah, int wl,
                            int reduce, int x, int y, int w, int h, char *msg, int cap)
{
    return say(rgb_frames_window_refusal(ctx_rgb != 0, cp, same_geometry != 0, n, r, g, b, streams, (size_t)pitch, (size_t)frame_stride,
                                         (size_t)stream_stride, max_stream_shorts(aw, ah), aw, ah, wl, reduce, x, y, w, h), msg, cap);
}
int emu_rgbp_images_refusal(int ctx_rgb, int cp, int same_geometry, int n, const void *streams, unsigned long long stream_stride, int aw, int ah,
                            int wl, int reduce, int x, int y, int w, int h, int layout, const void *data, unsigned long long pitch,
                            unsigned long long plane_stride, unsigned long long frame_stride, char *msg, int cap)
{
    return say(rgb_images_window_refusal(ctx_rgb != 0, cp, same_geometry != 0, n, streams, (size_t)stream_stride, max_stream_shorts(aw, ah), aw, ah,
                                         wl, reduce, x, y, w, h, layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride), msg, cap);
}

// picsong_decode_rgb_frames_reduced: the 3 n streams to n frames' planes at 1/2^reduce, frame f's frame_stride bytes after
// r / g / b.  fuse: the caller's switch (the library: no PICSONG_RGB_NOFUSE).
// Returns -1: refused, nothing run; else bit 0: the fused tail ran, bit 3: the lengths were damaged.
int emu_rgbp_decode_reduced(int n, const uint16_t *streams, unsigned long long stream_stride, int reduce, uint8_t *r, uint8_t *g, uint8_t *b,
                            unsigned long long frame_stride, int aw, int ah, int wl, int lossy, float qs, const int32_t *lut0,
                            const int32_t *lut1, const int32_t *lut2, const int *geo, float k, int n_tables, int fuse, int *flag)
{
    if (rgb_frames_reduced_refusal(true, 2, true, n, r, g, b, streams, (size_t)frame_stride, (size_t)stream_stride, max_stream_shorts(aw, ah), aw,
                                   ah, wl, reduce))
        return -1;
    Ctx c(n, true, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    DecodeReport rep;
    if (decode_rgb_frames(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, reduce, nullptr, c.c16(reduce), true, fuse != 0,
                          kLayoutPlanar3, r, g, b, 0, (size_t)frame_stride, &rep)) return -1;
    return (rep.rgb_tail ? 1 : 0) | (c.bad ? 8 : 0);
}

// picsong_decode_rgb_images_reduced on its reduced + emit route: the visible rw x rh pixels of the n frames at 1/2^reduce in
// `layout`.  Returns -1: refused, or reduced_emit_ok says the call takes the window route; else 0, bit 3: damaged lengths.
int emu_rgbp_images_reduced(int n, const uint16_t *streams, unsigned long long stream_stride, int reduce, int rw, int rh, int layout,
                            uint8_t *data, unsigned long long pitch, unsigned long long plane_stride, unsigned long long frame_stride, int aw,
                            int ah, int wl, int lossy, float qs, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2,
                            const int *geo, float k, int n_tables, int fuse, int *flag)
{
    if (rgb_images_window_refusal(true, 2, true, n, streams, (size_t)stream_stride, max_stream_shorts(aw, ah), aw, ah, wl, reduce, 0, 0, rw, rh,
                                  layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride) || !reduced_emit_ok(aw, reduce))
        return -1;
    Ctx c(n, true, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    const size_t pp = (size_t)(aw >> reduce) * (size_t)(ah >> reduce);
    std::vector<uint8_t> lay(3 * (size_t)n * pp + 64, 0x5A);
    uint8_t *const lay64 = (uint8_t *)(((uintptr_t)lay.data() + 63) & ~(uintptr_t)63);
    if (decode_rgb_images_reduced(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, reduce, c.c16(reduce), true, fuse != 0, lay64,
                                  layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, rw, rh)) return -1;
    return c.bad ? 8 : 0;
}

// picsong_decode_rgb_frames_window (layout = PLANAR3 with the three plane pointers) and picsong_decode_rgb_images_window:
// the w x h window at (x, y) of the n frames at 1/2^reduce in `layout`.
// Returns -1: refused, nothing run; else bit 0: the epilogue's vector form ran, bit 3: the lengths were damaged.
int emu_rgbp_decode_window(int n, const uint16_t *streams, unsigned long long stream_stride, int reduce, int x, int y, int w, int h,
                           int layout, uint8_t *d0, uint8_t *d1, uint8_t *d2, unsigned long long pitch, unsigned long long frame_stride,
                           int aw, int ah, int wl, int lossy, float qs, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2,
                           const int *geo, float k, int n_tables, int *flag)
{
    // (the frames call's planes as a PLANAR3 image would hold them, or the image call's own check)
    const char *why = layout == kLayoutPlanar3
        ? rgb_frames_window_refusal(true, 2, true, n, d0, d1, d2, streams, (size_t)pitch, (size_t)frame_stride, (size_t)stream_stride,
                                    max_stream_shorts(aw, ah), aw, ah, wl, reduce, x, y, w, h)
        : rgb_images_window_refusal(true, 2, true, n, streams, (size_t)stream_stride, max_stream_shorts(aw, ah), aw, ah, wl, reduce, x, y, w, h,
                                    layout, d0, (size_t)pitch, 0, (size_t)frame_stride);
    if (why) return -1;
    Ctx c(n, true, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    const WindowPlan plan = window_plan(aw, ah, wl, lossy != 0, reduce, x, y, w, h);
    DecodeReport rep;
    if (decode_rgb_frames(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, reduce, &plan, false, true, false, layout, d0, d1, d2,
                          (size_t)pitch, (size_t)frame_stride, &rep)) return -1;
    return (rep.vec ? 1 : 0) | (c.bad ? 8 : 0);
}

}  // extern "C"
