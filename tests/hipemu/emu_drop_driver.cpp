// TEST INFRASTRUCTURE ONLY -- the reduced-quality decode (picsong_ctx_set_decode_drop) on the CPU wave emulator: the
// library's own sequences (launch_decoder, decode_frames, decode_rgb_frames, launch_seq.hpp) over a context of
// emu_decode_ctx.hpp's making with BpcArgs::drop set after its construction, the choice of kernel, grid and scratch
// (kernel_select.hpp) and the kernel sources of cuda-image-and-video-codec_amd/csrc/picsong_hip.hip, run through the
// emulator's launcher.  The context poisons the plane scratch: a result equal to the expected one read no undecoded plane.
// Built by tests/test_drop_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include "emu_decode_ctx.hpp"

extern "C" {

int emu_drop_launches(void) { return g_launches; }
void emu_drop_reset(void) { g_launches = 0; }

// the host rule (picsong_drop_planes) and, beside it, the level the kernels' own find_subband gives the codeblock's corner
int emu_drop_planes(int aw, int ah, int wl, int drop, int cb) { return drop_planes_of(aw, ah, wl, drop, cb); }
int emu_drop_kernel_level(int aw, int ah, int wl, int cb)
{
    int level, sb;
    find_subband((cb % (aw / 64)) * 64, (cb / (aw / 64)) * 64, aw, ah, wl, level, sb);
    return level;
}
int emu_drop_ok(int drop) { return drop_ok(drop) ? 1 : 0; }

// select_decoder with and without its last parameter.  Bit i (i = from_stream + 2 * c16 over the three k = 0 forms, and
// bit 4 / 5 for a -k > 0 / -cp 3 launch from the stream): drop = false returns the function pointer, threads, workgroups
// and scratch the call without the parameter returns.  Bits 8 + i: drop = true returns ANOTHER kernel on the same grid
// and scratch (i = 0..2), none at all (-k > 0, -cp 3).
int emu_drop_selector(unsigned waves)
{
    int bits = 0;
    auto same = [](const BpcLaunch &x, const BpcLaunch &y) { return x.kernel == y.kernel && x.threads == y.threads && x.wgs == y.wgs && x.scratch_dwords == y.scratch_dwords; };
    const bool forms[3][2] = { { false, false }, { true, false }, { true, true } };
    for (int i = 0; i < 3; i++) {
        const BpcLaunch old = select_decoder(false, false, false, forms[i][0], forms[i][1], waves);
        const BpcLaunch off = select_decoder(false, false, false, forms[i][0], forms[i][1], waves, false);
        const BpcLaunch on = select_decoder(false, false, false, forms[i][0], forms[i][1], waves, true);
        if (old.kernel && same(old, off)) bits |= 1 << i;
        if (on.kernel && on.kernel != old.kernel && on.threads == old.threads && on.wgs == old.wgs && on.scratch_dwords == old.scratch_dwords) bits |= 1 << (8 + i);
    }
    if (same(select_decoder(false, true, false, true, false, waves), select_decoder(false, true, false, true, false, waves, false))) bits |= 1 << 4;
    if (same(select_decoder(true, false, false, false, false, waves), select_decoder(true, false, false, false, false, waves, false))) bits |= 1 << 5;
    if (!select_decoder(false, true, false, true, false, waves, true).kernel) bits |= 1 << 12;
    if (!select_decoder(true, false, false, false, false, waves, true).kernel) bits |= 1 << 13;
    // (the three drop kernels are three kernels)
    if (select_decoder(false, false, false, false, false, waves, true).kernel != select_decoder(false, false, false, true, false, waves, true).kernel &&
        select_decoder(false, false, false, true, false, waves, true).kernel != select_decoder(false, false, false, true, true, waves, true).kernel) bits |= 1 << 14;
    return bits;
}

// The decoder alone, as picsong_bpc_decode (staging / sizes: the 32-bit staging form) or as the frame paths' head runs it
// (stream: the intake's scan, then the decoder on the packed stream itself), every codeblock, 32-bit coefficients into
// `coef` (AW * AH int32, filled by the caller).  Returns -1 on a refused launch, else bit 3: the lengths were damaged.
int emu_drop_decode_coeffs(const int32_t *staging, const int32_t *sizes, const uint16_t *stream, unsigned stream_shorts, int aw, int ah,
                           int wl, const int32_t *lut, const int *geo, int drop, int32_t *coef, int *flag)
{
    Ctx c(1, false, aw, ah, wl, 0, 1.0f, lut, nullptr, nullptr, geo, 0.0f, 1, flag, stream_shorts, false, coef);
    c.a.drop = drop;
    const unsigned waves = (unsigned)(c.g.ncb + 1) / 2;
    if (stream) {
        if (stream_intake(go, stream, 1, stream_shorts, true, c.g.ncb, c.g.P, c.w, c.g.flag)) return -1;
    } else {
        c.w.staging = const_cast<int32_t *>(staging); c.w.sizes = const_cast<int32_t *>(sizes);
    }
    if (launch_decoder(go, c.a, false, waves, false, c.w, stream, stream_shorts, stream_shorts, false)) return -1;
    return c.bad ? 8 : 0;
}

// n grey frames under `drop` through decode_frames: whole (r = 0, win = 0), at 1/2^r, or the window x, y, w, h of that
// image (row stride pitch).  coef: the decoder's output arrays (n x AW * AH int32), filled by the caller.
// Returns -1: a launch failed; else bit 0: level r wrote the pixels, bit 1: the 16-bit coefficient form, bit 2: levels
// r + 1 and r ran as one launch, bit 3: the lengths were damaged.
int emu_drop_decode(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, int lossy, float qs, const int32_t *lut,
                    const int *geo, int want_c16, int drop, int r, int win, int x, int y, int w, int h, int32_t *coef, uint8_t *pixels,
                    size_t pitch, int *flag, int n, size_t frame_stride)
{
    Ctx c(n, false, aw, ah, wl, lossy, qs, lut, nullptr, nullptr, geo, 0.0f, 1, flag, stream_shorts, false, coef);
    c.a.drop = drop;
    DecodeReport rep;
    int rc;
    if (win) {
        const WindowPlan plan = window_plan(aw, ah, wl, lossy != 0, r, x, y, w, h);
        rc = decode_frames(go, c.g, c.a, c.w, (unsigned)n, stream, stream_shorts, r, &plan, false, true, pixels, frame_stride, pitch, &rep);
    } else {
        rc = decode_frames(go, c.g, c.a, c.w, (unsigned)n, stream, stream_shorts, r, nullptr, want_c16 && c.c16(r), true, pixels, frame_stride, 0, &rep);
    }
    if (rc) return -1;
    return (rep.pixels ? 1 : 0) | (rep.c16 ? 2 : 0) | (rep.fused10 ? 4 : 0) | (c.bad ? 8 : 0);
}

// n RGB frames under `drop` through decode_rgb_frames (the three components' tables on one grid): the 3 n streams to the
// frames' planes of (aw >> r) x (ah >> r) bytes, frame f's frame_stride bytes after r / g / b.
// Returns -1: a launch failed; else bit 0: the fused tail ran, bit 1: 16-bit coefficients.
int emu_drop_decode_rgb(int n, const uint16_t *streams, unsigned long long stream_stride, uint8_t *r, uint8_t *g, uint8_t *b,
                        unsigned long long frame_stride, int aw, int ah, int wl, int lossy, float qs, const int32_t *lut0, const int32_t *lut1,
                        const int32_t *lut2, const int *geo, int drop, int reduce, int *flag)
{
    Ctx c(n, true, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, 0.0f, 1, flag, (uint32_t)max_stream_shorts(aw, ah));
    c.a.drop = drop;
    DecodeReport rep;
    if (decode_rgb_frames(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, reduce, nullptr, c.c16(reduce), true, true, kLayoutPlanar3,
                          r, g, b, 0, (size_t)frame_stride, &rep)) return -1;
    return (rep.rgb_tail ? 1 : 0) | (rep.c16 ? 2 : 0);
}

}  // extern "C"
