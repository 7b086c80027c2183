// TEST INFRASTRUCTURE ONLY -- the n-frame RGB proxy calls (picsong_decode_rgb_frames_reduced / _window,
// picsong_decode_rgb_images_reduced / _window) on the CPU wave emulator: their argument checks (kernel_select.hpp) and the
// launch sequences the library runs (decode_rgb_frames_reduced and decode_rgb_frames_window, launch_seq.hpp), through a
// launcher that counts its launches.  What is written here is what picsong_hip.hip keeps in a context: the buffers
// (poisoned) and the switches.
// Built by tests/test_rgb_proxy_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static int g_launches = 0;
struct CountGo {
    template <typename K, typename... A>
    int operator()(K k, dim3 grid, unsigned threads, const A &...args) const
    {
        g_launches++;
        return emu::Go{}(k, grid, threads, args...);
    }
};
static const CountGo go{};

static size_t max_stream_shorts(int aw, int ah) { return 9 + 2 * (size_t)(aw / 64) * (size_t)(ah / 64) + (size_t)aw * (size_t)ah + 1; }

static int say(const char *why, char *msg, int cap)
{
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

// a context of 3 n planes: its buffers, poisoned, and what rgb_proxy_begin (picsong_hip.hip) hands the sequences
struct Ctx {
    std::vector<int32_t> coef_i, work, sizes, offsets, totals;
    std::vector<uint32_t> scratch;
    Workspace w;
    RgbProxyCtx g;
    BpcArgs a;
    int bad = 0;
    Ctx(int n, int aw, int ah, int wl, int lossy, float qs, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2, const int *geo,
        float k, int n_tables, int *flag)
    {
        const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
        const int ncb = (aw / 64) * (ah / 64);
        const unsigned np = 3u * (unsigned)n;
        coef_i.assign((size_t)np * P, 0x5A5A5A5A); work.assign((size_t)np * (P + extra), 0x5A5A5A5A);
        sizes.assign((size_t)np * ncb, -7); offsets.assign((size_t)np * ncb, -7); totals.assign(np, -7);
        // (whole workgroups a plane, every codeblock pair or the most a window lists: dec_waves of a context)
        const unsigned wpf = (unsigned)std::max(rgb_component_waves(k > 0.0f, (ncb + 1) / 2), window_waves_cap(aw, ah, wl, lossy != 0, ncb, 4));
        scratch.assign(decoder_scratch_dwords(false, k > 0.0f, np * wpf), 0xDEADBEEFu);
        w = Workspace{ work.data(), nullptr, sizes.data(), offsets.data(), totals.data(), scratch.data(), coef_i.data() };
        a = bpc_frame_args(aw, ah, wl, lut0, lut_geo(geo), flag);
        a.k = k; a.n_tables = n_tables;
        const int32_t *luts[3] = { lut0, lut1, lut2 };
        for (int c = 0; c < 3; c++) { a.lut_c[c] = luts[c]; a.img_c[c] = nullptr; }
        bool compact = k > 0.0f && bulk_compact(aw, ah, wl, lut_geo(geo));
        if (const char *e = getenv("PICSONG_BULK_FULLTAB")) if (atoi(e) != 0) compact = false;
        g.aw = aw; g.ah = ah; g.wl = wl; g.ncb = ncb;
        g.lossy = lossy != 0; g.qs = qs; g.fast_div = lossy && dequant_fast_ok(qs, wl); g.off = 128;
        g.P = P; g.extra = extra; g.direct = true; g.compact = compact;
        g.max_stream = (uint32_t)max_stream_shorts(aw, ah); g.flag = &bad;
    }
};

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
    Ctx c(n, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag);
    bool fused = false;
    if (decode_rgb_frames_reduced(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, reduce,
                                  dec_c16_ok(lossy != 0, wl, qs, 255, aw, ah, c.g.fast_div, reduce), true, fuse != 0, r, g, b, frame_stride,
                                  &fused)) return -1;
    return (fused ? 1 : 0) | (c.bad ? 8 : 0);
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
    Ctx c(n, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag);
    const size_t pp = (size_t)(aw >> reduce) * (size_t)(ah >> reduce);
    std::vector<uint8_t> lay(3 * (size_t)n * pp + 64, 0x5A);
    uint8_t *const lay64 = (uint8_t *)(((uintptr_t)lay.data() + 63) & ~(uintptr_t)63);
    if (decode_rgb_images_reduced(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, reduce,
                                  dec_c16_ok(lossy != 0, wl, qs, 255, aw, ah, c.g.fast_div, reduce), true, fuse != 0, lay64, layout, data,
                                  (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, rw, rh)) return -1;
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
    Ctx c(n, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag);
    const WindowPlan plan = window_plan(aw, ah, wl, lossy != 0, reduce, x, y, w, h);
    bool vec = false;
    if (decode_rgb_frames_window(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, plan, layout, d0, d1, d2, (size_t)pitch,
                                 (size_t)frame_stride, &vec)) return -1;
    return (vec ? 1 : 0) | (c.bad ? 8 : 0);
}

}  // extern "C"
