// TEST INFRASTRUCTURE ONLY -- batched RGB frames (picsong_encode_rgb_frames / picsong_decode_rgb_frames) on the CPU wave
// emulator: the argument checks (rgb_frames_refusal / rgb_images_refusal, kernel_select.hpp) and the launch sequences the
// library runs (rgb_forward_transform with n, the coder launch over 3 n planes, pack_rgb_frames; decode_rgb_frames),
// through a launcher that counts its launches.  What a context keeps -- the buffers (poisoned), the tables, the switches
// -- is emu_decode_ctx.hpp's.
// Built by tests/test_rgb_frames_emulated.py with the flags of tests/hipemu/Makefile.
#include "emu_decode_ctx.hpp"

extern "C" {

int emu_rgbf_launches(void) { return g_launches; }
void emu_rgbf_reset(void) { g_launches = 0; }

// 1 and the reason in msg when the frame calls refuse these arguments, else 0
int emu_rgbf_refusal(int ctx_rgb, int cp, int same_geometry, int n, const void *r, const void *g, const void *b, const void *streams,
                     unsigned long long frame_stride, unsigned long long stream_stride, int aw, int ah, char *msg, int cap)
{
    const char *why = rgb_frames_refusal(ctx_rgb != 0, cp, same_geometry != 0, n, r, g, b, streams, (size_t)frame_stride, (size_t)stream_stride,
                                         (size_t)aw * (size_t)ah, max_stream_shorts(aw, ah));
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}
// ... and the image calls
int emu_rgbf_images_refusal(int layout, const void *data, unsigned long long pitch, unsigned long long plane_stride,
                            unsigned long long frame_stride, int n, int w, int h, int aw, int ah, char *msg, int cap)
{
    const char *why = rgb_images_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, n, w, h, aw, ah);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

// picsong_encode_rgb_frames.  luts: the three component tables (n_tables each, one geometry `geo`); header: the nine
// populated header shorts; fuse: the caller's switch (the library: aligned planes, no PICSONG_RGB_NOFUSE).
// Out: the 3 n streams stream_stride shorts apart, totals[3 n]; and, where not null, what the stages left: coef (3 n
// buffers of coef_z = 4 (P + extra) bytes, an int16 Mallat array at each one's start when bit 1 of the result is set),
// staging16 (3 n x P shorts), sizes (3 n x nCB).  stages = 1: the transform only (no stream is written); else all three.
// Returns -1: refused, nothing run; else bit 0: the fused head ran, bit 1: 16-bit coefficients.
int emu_rgbf_encode(int ctx_rgb, int cp, int n, const uint8_t *r, const uint8_t *g, const uint8_t *b, unsigned long long frame_stride,
                    int first_iter, int header_mask, uint16_t *streams, unsigned long long stream_stride, int aw, int ah, int wl, int lossy,
                    float qs, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2, const int *geo, float k, int n_tables,
                    const uint16_t *header, int fuse, int stages, int32_t *totals, void *coef_out, uint16_t *staging_out, int32_t *sizes_out, int *flag)
{
    if (rgb_frames_refusal(ctx_rgb != 0, cp, true, n, r, g, b, streams, (size_t)frame_stride, (size_t)stream_stride, (size_t)aw * (size_t)ah,
                           max_stream_shorts(aw, ah)))
        return -1;
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), coef_z = (P + extra) * 4;
    const int ncb = (aw / 64) * (ah / 64);
    const unsigned np = 3u * (unsigned)n;
    std::vector<int32_t> coef((size_t)np * (P + extra), 0x5A5A5A5A), planes((size_t)np * P, 0x5A5A5A5A);
    const bool c16ctx = coef16_ok(lossy != 0, wl, qs, 255) && dwt_c16_geometry_ok(aw, ah, wl);
    auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward(src, u8in, coef.data(), aw, ah, wl, qs, c16ctx); };
    const bool aligned = ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b)) & 15u) == 0 && (n == 1 || (frame_stride & 15u) == 0);
    bool c16 = false, fused = false;
    if (rgb_forward_transform(go, lossy != 0, c16ctx && aligned && fuse != 0, plan_of, true, r, g, b, planes.data(), P, 128, coef_z, &c16, &fused,
                              (unsigned)n, frame_stride)) return -1;
    if (coef_out) memcpy(coef_out, coef.data(), coef.size() * 4);
    if (stages < 2) return (fused ? 1 : 0) | (c16 ? 2 : 0);

    const int32_t *luts[3] = { lut0, lut1, lut2 };
    // (the three component tables on one coder grid of 3 n planes: bpc_args_rgb + rgb_frames_args, picsong_hip.hip)
    BpcArgs a = table_args(aw, ah, wl, luts, geo, k, n_tables, flag);
    a.frames = (int)np; a.waves_per_frame = rgb_component_waves(k > 0.0f, (ncb + 1) / 2);
    const unsigned waves = np * (unsigned)a.waves_per_frame;
    std::vector<uint16_t> st16((size_t)np * P, 0xDEADu);
    std::vector<int32_t> sizes((size_t)np * ncb, -7), offsets((size_t)np * ncb, -7);
    std::vector<uint32_t> scratch(encoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    a.c16 = c16 ? 1 : 0; a.coeffs_in = coef.data(); a.is_float = lossy ? 1 : 0; a.coef_z = coef_z;
    a.staging16 = st16.data(); a.sizes = sizes.data(); a.plane_scratch = scratch.data();
    if (launch_encoder(go, a, false, emu_compact(aw, ah, wl, geo, k), waves)) return -1;
    if (staging_out) memcpy(staging_out, st16.data(), st16.size() * 2);
    if (sizes_out) memcpy(sizes_out, sizes.data(), sizes.size() * 4);

    const Workspace w = { nullptr, nullptr, sizes.data(), offsets.data(), totals, nullptr, nullptr };
    if (pack_rgb_frames(go, st16.data(), w, ncb, (unsigned)n, header, first_iter, header_mask, streams, P, (size_t)stream_stride)) return -1;
    return (fused ? 1 : 0) | (c16 ? 2 : 0);
}

// picsong_decode_rgb_frames: the 3 n streams to n frames' pixel planes, frame f's frame_stride bytes after r / g / b.
// fuse: the caller's switch (the library: no PICSONG_RGB_NOFUSE).
// Returns -1: refused, nothing run; else bit 0: a fused tail ran, bit 1: 16-bit coefficients.
int emu_rgbf_decode(int ctx_rgb, int cp, int n, const uint16_t *streams, unsigned long long stream_stride, uint8_t *r, uint8_t *g, uint8_t *b,
                    unsigned long long frame_stride, int aw, int ah, int wl, int lossy, float qs, const int32_t *lut0, const int32_t *lut1,
                    const int32_t *lut2, const int *geo, float k, int n_tables, int fuse, int *flag)
{
    if (rgb_frames_refusal(ctx_rgb != 0, cp, true, n, r, g, b, streams, (size_t)frame_stride, (size_t)stream_stride, (size_t)aw * (size_t)ah,
                           max_stream_shorts(aw, ah)))
        return -1;
    Ctx c(n, true, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    DecodeReport rep;
    if (decode_rgb_frames(go, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, 0, nullptr, c.c16(0), true, fuse != 0, kLayoutPlanar3,
                          r, g, b, 0, (size_t)frame_stride, &rep)) return -1;
    return (rep.rgb_tail ? 1 : 0) | (rep.c16 ? 2 : 0);
}

}  // extern "C"
