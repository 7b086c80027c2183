// TEST INFRASTRUCTURE ONLY -- batched RGB frames (picsong_encode_rgb_frames / picsong_decode_rgb_frames) on the CPU wave
// emulator: the argument checks (rgb_frames_refusal / rgb_images_refusal, kernel_select.hpp) and the launch sequences the
// library runs (rgb_forward_transform and run_inverse_rgb with n, the coder launches over 3 n planes, pack_rgb_frames,
// stream_intake), through a launcher that counts its launches.  What is written here is what picsong_hip.hip keeps in a
// context: the buffers (poisoned) and the switches.
// Built by tests/test_rgb_frames_emulated.py with the flags of tests/hipemu/Makefile.
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

// the three component tables on one coder grid of 3 n planes (bpc_args_rgb + rgb_frames_args, picsong_hip.hip)
static BpcArgs rgb_args(int aw, int ah, int wl, const int32_t *const *luts, const int *geo, float k, int n_tables, int n, int wpf,
                        int *flag)
{
    BpcArgs a = bpc_frame_args(aw, ah, wl, luts[0], lut_geo(geo), flag);
    a.k = k; a.n_tables = n_tables;
    for (int c = 0; c < 3; c++) { a.lut_c[c] = luts[c]; a.img_c[c] = nullptr; }
    a.cb_base = 0;
    a.frames = 3 * n; a.waves_per_frame = rgb_component_waves(k > 0.0f, wpf);
    return a;
}
static bool emu_compact(int aw, int ah, int wl, const int *geo)
{
    if (const char *e = getenv("PICSONG_BULK_FULLTAB")) if (atoi(e) != 0) return false;
    return bulk_compact(aw, ah, wl, lut_geo(geo));
}

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
    BpcArgs a = rgb_args(aw, ah, wl, luts, geo, k, n_tables, n, (ncb + 1) / 2, flag);
    const unsigned waves = np * (unsigned)a.waves_per_frame;
    std::vector<uint16_t> st16((size_t)np * P, 0xDEADu);
    std::vector<int32_t> sizes((size_t)np * ncb, -7), offsets((size_t)np * ncb, -7);
    std::vector<uint32_t> scratch(encoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    a.c16 = c16 ? 1 : 0; a.coeffs_in = coef.data(); a.is_float = lossy ? 1 : 0; a.coef_z = coef_z;
    a.staging16 = st16.data(); a.sizes = sizes.data(); a.plane_scratch = scratch.data();
    if (launch_encoder(go, a, false, k > 0.0f && emu_compact(aw, ah, wl, geo), waves)) return -1;
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
    if (n == 1) frame_stride = 0;
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
    const int ncb = (aw / 64) * (ah / 64);
    const unsigned np = 3u * (unsigned)n;
    std::vector<int32_t> coef_i((size_t)np * P, 0x5A5A5A5A), work((size_t)np * (P + extra), 0x5A5A5A5A);
    std::vector<int32_t> sizes((size_t)np * ncb, -7), offsets((size_t)np * ncb, -7), totals(np, -7);
    const int32_t *luts[3] = { lut0, lut1, lut2 };
    BpcArgs a = rgb_args(aw, ah, wl, luts, geo, k, n_tables, n, (ncb + 1) / 2, flag);
    const unsigned waves = np * (unsigned)a.waves_per_frame;
    std::vector<uint32_t> scratch(decoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    const Workspace w = { work.data(), nullptr, sizes.data(), offsets.data(), totals.data(), scratch.data(), coef_i.data() };
    int bad = 0;
    if (stream_intake(go, streams, np, (size_t)stream_stride, true, ncb, P, w, &bad)) return -1;
    const bool fast = lossy && dequant_fast_ok(qs, wl);
    const std::vector<InvLaunch> plan = plan_inverse_frames(coef_i.data(), work.data(), nullptr, nullptr, np, 0,
                                                            dec_c16_ok(lossy != 0, wl, qs, 255, aw, ah, fast), true, 0, aw, ah, wl, qs, fast, 128,
                                                            P, extra);
    const bool c16 = plan_inv_is_c16(plan);
    a.coef_z = (unsigned long long)P * (c16 ? 2ull : 4ull);
    if (launch_decoder(go, a, false, waves, k > 0.0f && emu_compact(aw, ah, wl, geo), w, streams, (size_t)stream_stride,
                       (uint32_t)max_stream_shorts(aw, ah), c16)) return -1;
    const bool px_aligned = ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b) | frame_stride) & 3u) == 0;
    if (inv_rgb_tail_ok(plan, lossy != 0) && px_aligned && fuse != 0) {
        if (run_inverse_rgb(go, lossy != 0, true, plan, 128, r, g, b, (unsigned)n, frame_stride)) return -1;
        return 1 | (c16 ? 2 : 0);
    }
    if (run_inverse(go, lossy != 0, true, plan, np)) return -1;
    const size_t z = (P + extra) * 4;
    for (int f = 0; f < n; f++) {
        const char *img = (const char *)plan.back().a.dst + (size_t)(3 * f) * z;
        const size_t at = (size_t)f * (size_t)frame_stride;
        if (rgb_inverse(go, lossy != 0, img, img + z, img + 2 * z, r + at, g + at, b + at, P / 4, 128)) return -1;
    }
    return c16 ? 2 : 0;
}

}  // extern "C"
