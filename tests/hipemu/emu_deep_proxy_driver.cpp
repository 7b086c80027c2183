// TEST INFRASTRUCTURE ONLY -- the deep proxy calls (picsong_decode_frames16_reduced / _window,
// picsong_decode_rgb_frames16_reduced / _window, the 16-bit layouts of picsong_decode_rgb_images_window / _reduced) on the CPU
// wave emulator: their argument checks (kernel_select.hpp) and the launch sequences the library runs (decode_frames and
// decode_rgb_frames with DecodeCtx::px_max, launch_seq.hpp), through a launcher that records which kernels it was handed.
// What a context keeps -- the buffers (poisoned), the tables, the switches -- is emu_decode_ctx.hpp's, with g.off and
// g.px_max set to the depth's; PICSONG_DEEP_NOFUSE is read at every call.
// Built by tests/test_deep_proxy_emulated.py with the flags of tests/hipemu/Makefile -- as a shared library, and, with
// -DEMU_DEEP_PROXY_MAIN and the sanitizers, as a stand-alone program that replays recorded calls on heap buffers of exactly
// the documented sizes (main, below).
#include "emu_decode_ctx.hpp"

#include <string>

static std::vector<const void *> g_log;
struct RecordGo {
    template <typename K, typename... A>
    int operator()(K k, dim3 grid, unsigned threads, const A &...args) const
    {
        const void *p = reinterpret_cast<const void *>(k);
        bool seen = false;
        for (const void *q : g_log) seen = seen || q == p;
        if (!seen) g_log.push_back(p);
        return emu::Go{}(k, grid, threads, args...);
    }
};
static const RecordGo rgo{};

static int say(const char *why, char *msg, int cap)
{
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

struct Tables { const int32_t *lut0, *lut1, *lut2; const int *geo; float k; int n_tables; };

// the grey pair: win = 0 the reduced call, 1 the window call.  -1: refused or a launch failed; else bit 0: level `reduce`
// stored the samples itself (reduced call), bit 3: damaged lengths
static int grey_call(int n, const uint16_t *streams, size_t stream_stride, int reduce, int win, int x, int y, int w, int h, uint16_t *out,
                     size_t pitch, size_t frame_stride, int aw, int ah, int wl, int lossy, float qs, int bd, const Tables &t, int drop, int *flag)
{
    const char *why = win ? frames16_window_refusal(bd, false, 2, n, out, streams, pitch, frame_stride, stream_stride, max_stream_shorts(aw, ah), aw,
                                                    ah, wl, reduce, x, y, w, h)
                          : frames16_reduced_refusal(bd, false, 2, n, out, streams, frame_stride, stream_stride, max_stream_shorts(aw, ah), aw, ah, wl,
                                                     reduce);
    if (why) return -1;
    Ctx c(n, false, aw, ah, wl, lossy, qs, t.lut0, nullptr, nullptr, t.geo, t.k, t.n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    c.g.off = 1 << (bd - 1); c.g.px_max = (1 << bd) - 1;
    c.a.drop = drop;
    WindowPlan plan;
    if (win) plan = window_plan(aw, ah, wl, lossy != 0, reduce, x, y, w, h);
    DecodeReport rep;
    if (decode_frames(rgo, c.g, c.a, c.w, (unsigned)n, streams, stream_stride, reduce, win ? &plan : nullptr, false, true, (uint8_t *)out,
                      frame_stride, pitch, &rep)) return -1;
    return (rep.pixels ? 1 : 0) | (c.bad ? 8 : 0);
}

// the RGB pair (layout = PLANAR3_16 with the three plane pointers) and the image calls' window route (RGB48 / RGBA64, or
// PLANAR3_16 with plane_stride: d1 = d0 + plane_stride, d2 = d0 + 2 plane_stride, checked as an image where images != 0).
// -1: refused or a launch failed; else bit 0: the epilogue's vector form ran (window), bit 3: damaged lengths
static int rgb_call(int n, const uint16_t *streams, size_t stream_stride, int reduce, int win, int x, int y, int w, int h, int layout, int images,
                    uint8_t *d0, uint8_t *d1, uint8_t *d2, size_t pitch, size_t frame_stride, int aw, int ah, int wl, int lossy, float qs, int bd,
                    const Tables &t, int drop, int *flag)
{
    const size_t ms = max_stream_shorts(aw, ah);
    const char *why;
    if (images) why = rgb_images_window_refusal(true, 2, true, n, streams, stream_stride, ms, aw, ah, wl, reduce, x, y, w, h, layout, d0, pitch,
                                                (size_t)(d1 - d0), frame_stride, true);
    else if (win) why = rgb_frames16_window_refusal(bd, true, 2, true, n, d0, d1, d2, streams, pitch, frame_stride, stream_stride, ms, aw, ah, wl,
                                                    reduce, x, y, w, h);
    else why = rgb_frames16_reduced_refusal(bd, true, 2, true, n, d0, d1, d2, streams, frame_stride, stream_stride, ms, aw, ah, wl, reduce);
    if (why) return -1;
    Ctx c(n, true, aw, ah, wl, lossy, qs, t.lut0, t.lut1, t.lut2, t.geo, t.k, t.n_tables, flag, (uint32_t)ms);
    c.g.off = 1 << (bd - 1); c.g.px_max = (1 << bd) - 1;
    c.a.drop = drop;
    WindowPlan plan;
    if (win) plan = window_plan(aw, ah, wl, lossy != 0, reduce, x, y, w, h);
    DecodeReport rep;
    if (decode_rgb_frames(rgo, c.g, c.a, c.w, (unsigned)n, streams, stream_stride, reduce, win ? &plan : nullptr, false, true, true, layout, d0, d1,
                          d2, pitch, frame_stride, &rep)) return -1;
    return (rep.vec ? 1 : 0) | (c.bad ? 8 : 0);
}

extern "C" {

void emu_dpx_log_reset(void) { g_log.clear(); }
int emu_dpx_log_read(const void **ptrs, int cap)
{
    for (int i = 0; i < cap && i < (int)g_log.size(); i++) ptrs[i] = g_log[(size_t)i];
    return (int)g_log.size();
}

// Host only: every kernel the new selectors can return -- select_window_out's uint16 form and select_window_rgb16 (three
// layouts, both forms), 5/3 and 9/7.  The distinct pointers into ptrs, a label each.
int emu_dpx_selector_kernels(const void **ptrs, char *labels, int label_bytes, int cap)
{
    std::vector<const void *> seen;
    auto add = [&](const void *p, const std::string &label) {
        for (const void *q : seen) if (q == p) return;
        if ((int)seen.size() < cap) {
            ptrs[seen.size()] = p;
            snprintf(labels + seen.size() * (size_t)label_bytes, (size_t)label_bytes, "%s", label.c_str());
        }
        seen.push_back(p);
    };
    auto s = [](const char *name, int v) { return std::string(" ") + name + "=" + std::to_string(v); };
    for (int lossy = 0; lossy < 2; lossy++) {
        add(reinterpret_cast<const void *>(select_window_out(lossy != 0, kWinOutU16)), "window_u16" + s("lossy", lossy));
        const int layouts[3] = { kLayoutPlanar3_16, kLayoutRgb48, kLayoutRgba64 };
        for (int layout : layouts)
            for (int vec = 0; vec < 2; vec++) {
                uint8_t *const d = (uint8_t *)(uintptr_t)(vec ? 4096 : 4098);
                const WinRgb16Args a = window_rgb16_args(layout, (const void *)(uintptr_t)8192, 1024, 8, 8, d, d + 1024, d + 2048, 64, 0, 1, 256, 511);
                add(reinterpret_cast<const void *>(select_window_rgb16(lossy != 0, layout, a, 1).kernel),
                    "window_rgb16" + s("lossy", lossy) + s("layout", layout) + s("vec", vec));
            }
    }
    return (int)seen.size();
}

// Host only: is level `reduce` of a context of these parameters a vector launch?  (the one condition, beside the output's
// alignment and PICSONG_DEEP_NOFUSE, under which plan_inverse_frames lets it store the uint16 samples itself)
int emu_dpx_level_is_vector(int aw, int ah, int wl, int lossy, float qs, int reduce)
{
    std::vector<int32_t> buf(64);
    void *const p = (void *)(((uintptr_t)buf.data() + 63) & ~(uintptr_t)63);
    const std::vector<InvLaunch> plan = plan_dwt_inverse_reduced((const int32_t *)p, p, aw, ah, wl, qs, lossy && dequant_fast_ok(qs, wl), false, reduce);
    return !plan.empty() && plan.back().vec ? 1 : 0;
}

// 1 and the reason in msg when the calls refuse these arguments, else 0
int emu_dpx_grey_reduced_refusal(int bd, int ctx_rgb, int cp, int n, const void *out, const void *streams, unsigned long long frame_stride,
                                 unsigned long long stream_stride, int aw, int ah, int wl, int reduce, char *msg, int cap)
{
    return say(frames16_reduced_refusal(bd, ctx_rgb != 0, cp, n, out, streams, (size_t)frame_stride, (size_t)stream_stride, max_stream_shorts(aw, ah),
                                        aw, ah, wl, reduce), msg, cap);
}
int emu_dpx_grey_window_refusal(int bd, int ctx_rgb, int cp, int n, const void *out, const void *streams, unsigned long long pitch,
                                unsigned long long frame_stride, unsigned long long stream_stride, int aw, int ah, int wl, int reduce, int x,
                                int y, int w, int h, char *msg, int cap)
{
    return say(frames16_window_refusal(bd, ctx_rgb != 0, cp, n, out, streams, (size_t)pitch, (size_t)frame_stride, (size_t)stream_stride,
                                       max_stream_shorts(aw, ah), aw, ah, wl, reduce, x, y, w, h), msg, cap);
}
int emu_dpx_rgb_reduced_refusal(int bd, int ctx_rgb, int cp, int same_geometry, int n, const void *r, const void *g, const void *b,
                                const void *streams, unsigned long long frame_stride, unsigned long long stream_stride, int aw, int ah, int wl,
                                int reduce, char *msg, int cap)
{
    return say(rgb_frames16_reduced_refusal(bd, ctx_rgb != 0, cp, same_geometry != 0, n, r, g, b, streams, (size_t)frame_stride, (size_t)stream_stride,
                                            max_stream_shorts(aw, ah), aw, ah, wl, reduce), msg, cap);
}
int emu_dpx_rgb_window_refusal(int bd, int ctx_rgb, int cp, int same_geometry, int n, const void *r, const void *g, const void *b,
                               const void *streams, unsigned long long pitch, unsigned long long frame_stride, unsigned long long stream_stride,
                               int aw, int ah, int wl, int reduce, int x, int y, int w, int h, char *msg, int cap)
{
    return say(rgb_frames16_window_refusal(bd, ctx_rgb != 0, cp, same_geometry != 0, n, r, g, b, streams, (size_t)pitch, (size_t)frame_stride,
                                           (size_t)stream_stride, max_stream_shorts(aw, ah), aw, ah, wl, reduce, x, y, w, h), msg, cap);
}
int emu_dpx_images_refusal(int ctx_rgb, int deep_rgb, int cp, int same_geometry, int n, const void *streams, unsigned long long stream_stride,
                           int aw, int ah, int wl, int reduce, int x, int y, int w, int h, int layout, const void *data, unsigned long long pitch,
                           unsigned long long plane_stride, unsigned long long frame_stride, char *msg, int cap)
{
    return say(rgb_images_window_refusal(ctx_rgb != 0, cp, same_geometry != 0, n, streams, (size_t)stream_stride, max_stream_shorts(aw, ah), aw, ah,
                                         wl, reduce, x, y, w, h, layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride,
                                         deep_rgb != 0), msg, cap);
}

int emu_dpx_grey(int n, const uint16_t *streams, unsigned long long stream_stride, int reduce, int win, int x, int y, int w, int h, uint16_t *out,
                 unsigned long long pitch, unsigned long long frame_stride, int aw, int ah, int wl, int lossy, float qs, int bd,
                 const int32_t *lut, const int *geo, float k, int n_tables, int drop, int *flag)
{
    const Tables t = { lut, nullptr, nullptr, geo, k, n_tables };
    return grey_call(n, streams, (size_t)stream_stride, reduce, win, x, y, w, h, out, (size_t)pitch, (size_t)frame_stride, aw, ah, wl, lossy, qs, bd,
                     t, drop, flag);
}
int emu_dpx_rgb(int n, const uint16_t *streams, unsigned long long stream_stride, int reduce, int win, int x, int y, int w, int h, int layout,
                int images, uint8_t *d0, uint8_t *d1, uint8_t *d2, unsigned long long pitch, unsigned long long frame_stride, int aw, int ah,
                int wl, int lossy, float qs, int bd, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2, const int *geo, float k,
                int n_tables, int drop, int *flag)
{
    const Tables t = { lut0, lut1, lut2, geo, k, n_tables };
    return rgb_call(n, streams, (size_t)stream_stride, reduce, win, x, y, w, h, layout, images, d0, d1, d2, (size_t)pitch, (size_t)frame_stride, aw,
                    ah, wl, lossy, qs, bd, t, drop, flag);
}

// The cone synthesis and the stores alone, over int32 Mallat arrays of the caller's making (P words each): grey (planes = 1)
// the window's samples into d0; RGB (planes = 3) the three components' cones, then the epilogue in `layout`.
// Returns -1: a launch failed; else bit 0: the epilogue's vector form ran.
int emu_dpx_synthesis(const int32_t *coef, int planes, int aw, int ah, int wl, int lossy, float qs, int bd, int reduce, int x, int y, int w, int h,
                      int layout, uint8_t *d0, uint8_t *d1, uint8_t *d2, unsigned long long pitch)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), z = (P + extra) * 4;
    const int off = 1 << (bd - 1), mx = (1 << bd) - 1;
    std::vector<int32_t> work((size_t)planes * (P + extra) + 16, 0x5A5A5A5A);
    void *const wrk = (void *)(((uintptr_t)work.data() + 63) & ~(uintptr_t)63);
    const WindowPlan plan = window_plan(aw, ah, wl, lossy != 0, reduce, x, y, w, h);
    if (planes == 1)
        return run_window(rgo, lossy != 0, plan, coef, wrk, P, aw, ah, qs, off, 1u, (unsigned long long)P * 4ull, z, d0, (size_t)pitch, 0, mx) ? -1 : 0;
    if (run_window(rgo, lossy != 0, plan, coef, wrk, P, aw, ah, qs, off, 3u, (unsigned long long)P * 4ull, z, nullptr, 0, 0, mx)) return -1;
    const WinRgb16Args ra = window_rgb16_args(layout, wrk, z, w, h, d0, d1, d2, (size_t)pitch, 0, 1u, off, mx);
    const WinRgb16Launch l = select_window_rgb16(lossy != 0, layout, ra, 1u);
    if (!l.kernel || rgo(l.kernel, l.grid, 256u, ra)) return -1;
    return l.vec ? 1 : 0;
}

}  // extern "C"

#ifdef EMU_DEEP_PROXY_MAIN
// The stand-alone program: replays the calls recorded in argv[1] (written by tests/test_deep_proxy_emulated.py) with every
// caller-side array -- streams, tables, outputs -- a heap buffer of exactly the documented size, and compares the outputs with
// the recorded ones.  Built with -fsanitize=address,undefined: an access one byte outside any of them ends the run.
// The file: records of (int64 byte count, bytes) --
//   params  int32 { aw, ah, wl, lossy, bd, n_tables, n, n_calls } + float32 { qs, k } (as two more words)
//   geo     int32[9]      grey table, RGB tables 0..2 (int32 arrays)     grey streams, RGB streams (uint16, n resp. 3 n strides)
//   then a call: int32 { rgb, win, reduce, x, y, w, h, layout, images, pitch, plane_stride, frame_stride, out_bytes } and the
//   expected out_bytes bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool read_record(FILE *f, std::vector<char> &buf)
{
    long long nb = 0;
    if (fread(&nb, sizeof nb, 1, f) != 1 || nb < 0) return false;
    buf.resize((size_t)nb);
    return nb == 0 || fread(buf.data(), 1, (size_t)nb, f) == (size_t)nb;
}
// an exactly-sized heap copy (malloc: the sanitizer's red zones start at its last byte)
template <typename T> static T *heap_copy(const std::vector<char> &buf)
{
    T *p = (T *)malloc(buf.size() ? buf.size() : 1);
    memcpy(p, buf.data(), buf.size());
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<char> rec;
    if (!read_record(f, rec) || rec.size() != 10 * 4) return 3;
    int32_t p[8];
    float fl[2];
    memcpy(p, rec.data(), sizeof p);
    memcpy(fl, rec.data() + sizeof p, sizeof fl);
    const int aw = p[0], ah = p[1], wl = p[2], lossy = p[3], bd = p[4], n_tables = p[5], n = p[6], n_calls = p[7];
    if (!read_record(f, rec)) return 3;
    int *const geo = heap_copy<int>(rec);
    int32_t *luts[4];
    for (int i = 0; i < 4; i++) {
        if (!read_record(f, rec)) return 3;
        luts[i] = heap_copy<int32_t>(rec);
    }
    uint16_t *streams[2];
    for (int i = 0; i < 2; i++) {
        if (!read_record(f, rec)) return 3;
        if (rec.size() != (size_t)(i ? 3 : 1) * (size_t)n * max_stream_shorts(aw, ah) * 2) return 3;
        streams[i] = heap_copy<uint16_t>(rec);
    }
    int bad = 0;
    for (int k = 0; k < n_calls; k++) {
        if (!read_record(f, rec) || rec.size() != 13 * 4) return 3;
        int32_t c[13];
        memcpy(c, rec.data(), sizeof c);
        if (!read_record(f, rec) || rec.size() != (size_t)c[12]) return 3;
        uint8_t *const out = (uint8_t *)malloc(rec.size());
        memset(out, 0xA5, rec.size());
        int flag = 0, rc;
        if (c[0]) {
            const Tables t = { luts[1], luts[2], luts[3], geo, fl[1], n_tables };
            // (interleaved: one array; PLANAR3_16: the planes plane_stride bytes apart in it)
            rc = rgb_call(n, streams[1], max_stream_shorts(aw, ah), c[2], c[1], c[3], c[4], c[5], c[6], c[7], c[8], out, out + c[10], out + 2 * c[10],
                          (size_t)c[9], (size_t)c[11], aw, ah, wl, lossy, fl[0], bd, t, 0, &flag);
        } else {
            const Tables t = { luts[0], nullptr, nullptr, geo, fl[1], n_tables };
            rc = grey_call(n, streams[0], max_stream_shorts(aw, ah), c[2], c[1], c[3], c[4], c[5], c[6], (uint16_t *)out, (size_t)c[9], (size_t)c[11],
                           aw, ah, wl, lossy, fl[0], bd, t, 0, &flag);
        }
        if (rc < 0 || (rc & 8) || flag || memcmp(out, rec.data(), rec.size()) != 0) {
            fprintf(stderr, "call %d: rc %d flag %d %s\n", k, rc, flag, rc >= 0 ? "or other bytes than recorded" : "");
            bad++;
        }
        free(out);
    }
    fclose(f);
    for (int i = 0; i < 2; i++) free(streams[i]);
    for (int i = 0; i < 4; i++) free(luts[i]);
    free(geo);
    printf("%d calls, %d bad\n", n_calls, bad);
    return bad ? 1 : 0;
}
#endif
