// TEST INFRASTRUCTURE ONLY -- deep RGB contexts (bit_depth 9..16, three uint16 planes a frame) on the CPU wave emulator: the
// library's own plans (plan_dwt_forward_rgb16, plan_inverse_frames with px_max), selectors (select_fwd) and launch
// sequences (rgb_forward16, rgb_inverse16, deep_rgb_forward, launch_encoder, pack_rgb_frames, decode_rgb_frames;
// launch_seq.hpp) over the kernel sources of cuda-image-and-video-codec_amd/csrc, through a launcher that records which
// kernels it was handed.  What a context keeps -- the buffers (poisoned), the tables, the switches -- is
// emu_decode_ctx.hpp's; PICSONG_DEEP_NOFUSE and PICSONG_DWT_BANDS are read at every call.
// Built by tests/test_deep_rgb_emulated.py with the flags of tests/hipemu/Makefile.
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

extern "C" {

void emu_drgb_log_reset(void) { g_log.clear(); }
int emu_drgb_log_read(const void **ptrs, int cap)
{
    for (int i = 0; i < cap && i < (int)g_log.size(); i++) ptrs[i] = g_log[(size_t)i];
    return (int)g_log.size();
}

// Host only: every kernel the selectors can return for a deep RGB launch that no other context takes -- select_fwd with
// FwdLaunch::rgb16 (band, vec, lossy) and the four element-wise transforms.  The distinct pointers into ptrs, a label each.
int emu_drgb_selector_kernels(const void **ptrs, char *labels, int label_bytes, int cap)
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
    const int bands[4] = { 4, 8, 16, 32 };
    for (int band : bands)
        for (int lossy = 0; lossy < 2; lossy++)
            for (int vec = 0; vec < 2; vec++) {
                FwdLaunch f;
                memset(&f, 0, sizeof f);
                f.band = band; f.vec = vec != 0; f.rgb16 = true;
                if (!vec && band > kRgb16ColumnMaxBand) continue;        // (plan_dwt_forward_rgb16 never asks for it)
                add(reinterpret_cast<const void *>(select_fwd(lossy != 0, f)), "fwd_rgb16" + s("band", band) + s("lossy", lossy) + s("vec", vec));
            }
    const int layouts[3] = { kLayoutPlanar3_16, kLayoutRgb48, kLayoutRgba64 };
    for (int layout : layouts)
        for (int vec = 0; vec < 2; vec++) {
            LayoutArgs a;
            memset(&a, 0, sizeof a);
            a.img = (uint8_t *)(uintptr_t)(vec ? 4096 : 4098); a.pad = (uint8_t *)(uintptr_t)8192; a.pitch = 2048;
            a.W = 200; a.H = 136; a.AW = 256; a.AH = 192;
            add(reinterpret_cast<const void *>(select_ingest(layout, a).kernel), "ingest_rgb16" + s("layout", layout) + s("vec", vec));
            add(reinterpret_cast<const void *>(select_emit(layout, a).kernel), "emit_rgb16" + s("layout", layout) + s("vec", vec));
        }
    add(reinterpret_cast<const void *>(rgb_forward16_kernel<int32_t>), "rgb_forward16 lossy=0");
    add(reinterpret_cast<const void *>(rgb_forward16_kernel<float>), "rgb_forward16 lossy=1");
    add(reinterpret_cast<const void *>(rgb_inverse16_kernel<int32_t>), "rgb_inverse16 lossy=0");
    add(reinterpret_cast<const void *>(rgb_inverse16_kernel<float>), "rgb_inverse16 lossy=1");
    return (int)seen.size();
}

// picsong_rgb_forward16 / picsong_rgb_inverse16 over n frames: sample planes smp_z bytes a frame apart, T planes cmp_z
int emu_drgb_transform_fwd(const uint16_t *r, const uint16_t *g, const uint16_t *b, void *c0, void *c1, void *c2, size_t n4, int lossy, int bd,
                           int n, unsigned long long smp_z, unsigned long long cmp_z)
{
    return rgb_forward16(rgo, lossy != 0, r, g, b, c0, c1, c2, n4, 1 << (bd - 1), (unsigned)n, smp_z, cmp_z);
}
int emu_drgb_transform_inv(const void *c0, const void *c1, const void *c2, uint16_t *r, uint16_t *g, uint16_t *b, size_t n4, int lossy, int bd,
                           int n, unsigned long long cmp_z, unsigned long long smp_z)
{
    return rgb_inverse16(rgo, lossy != 0, c0, c1, c2, r, g, b, n4, 1 << (bd - 1), (1 << bd) - 1, (unsigned)n, cmp_z, smp_z);
}

// The transform of picsong_encode_rgb_frames16: n frames' planes frame_stride bytes apart to 3 n coefficient buffers of
// P + extra elements (coef: 16-byte aligned).  Returns bit 0: level 0 applied the colour transform itself, bit 1: through its
// vector form; bits 8..: its band rows.
int emu_drgb_forward(const uint16_t *r, const uint16_t *g, const uint16_t *b, unsigned long long frame_stride, int n, void *coef, int aw, int ah,
                     int wl, int lossy, float qs, int bd)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
    std::vector<int32_t> planes((size_t)3 * n * P + 16, 0x5A5A5A5A);
    void *const pl = (void *)(((uintptr_t)planes.data() + 63) & ~(uintptr_t)63);
    bool in_kernel = false;
    if (deep_rgb_forward(rgo, lossy != 0, deep_nofuse(), r, g, b, (size_t)frame_stride, (unsigned)n, coef, pl, aw, ah, wl, qs, 1 << (bd - 1),
                         (unsigned long long)(P + extra) * 4ull, &in_kernel)) return -1;
    const FwdLaunch f = plan_dwt_forward_rgb16(r, g, b, n > 1 ? (size_t)frame_stride : 0, (unsigned)n, coef, aw, ah, wl, qs, 1 << (bd - 1))[0];
    return (in_kernel ? 1 : 0) | (in_kernel && f.vec ? 2 : 0) | (in_kernel ? f.band << 8 : 0);
}

// picsong_encode_rgb_frames16: transform, coder (32-bit coefficients, one grid over the 3 n planes, table z % 3), pack.
// Out: the 3 n streams stream_stride shorts apart, totals[3 n].  Returns -1: a launch failed; else emu_drgb_forward's bits.
int emu_drgb_encode(const uint16_t *r, const uint16_t *g, const uint16_t *b, unsigned long long frame_stride, int n, int first_iter,
                    int header_mask, uint16_t *streams, unsigned long long stream_stride, int32_t *totals, int aw, int ah, int wl, int lossy,
                    float qs, int bd, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2, const int *geo, float k, int n_tables,
                    const uint16_t *header, int *flag)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), coef_z = (P + extra) * 4;
    const int ncb = (aw / 64) * (ah / 64);
    const unsigned np = 3u * (unsigned)n;
    std::vector<int32_t> coef((size_t)np * (P + extra) + 16, 0x5A5A5A5A);
    void *const cf = (void *)(((uintptr_t)coef.data() + 63) & ~(uintptr_t)63);
    const int bits = emu_drgb_forward(r, g, b, frame_stride, n, cf, aw, ah, wl, lossy, qs, bd);
    if (bits < 0) return -1;
    const int32_t *luts[3] = { lut0, lut1, lut2 };
    BpcArgs a = table_args(aw, ah, wl, luts, geo, k, n_tables, flag);
    a.frames = (int)np; a.waves_per_frame = rgb_component_waves(k > 0.0f, (ncb + 1) / 2);
    const unsigned waves = np * (unsigned)a.waves_per_frame;
    std::vector<uint16_t> st16((size_t)np * P * 2, 0xDEADu);
    std::vector<int32_t> sizes((size_t)np * ncb, -7), offsets((size_t)np * ncb, -7);
    std::vector<uint32_t> scratch(encoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    a.c16 = 0; a.cb_base = 0; a.nCB = ncb; a.coeffs_in = cf; a.is_float = lossy ? 1 : 0; a.coef_z = coef_z;
    a.staging16 = st16.data(); a.sizes = sizes.data(); a.plane_scratch = scratch.data();
    if (launch_encoder(rgo, a, false, emu_compact(aw, ah, wl, geo, k), waves)) return -1;
    const Workspace w = { nullptr, nullptr, sizes.data(), offsets.data(), totals, nullptr, nullptr };
    if (pack_rgb_frames(rgo, st16.data(), w, ncb, (unsigned)n, header, first_iter, header_mask, streams, P, (size_t)stream_stride)) return -1;
    return bits;
}

// picsong_decode_rgb_frames16 under the context's `drop`: decode_rgb_frames with DecodeCtx::px_max.  Returns -1: a launch
// failed; else bit 0: a fused tail ran (never), bit 1: 16-bit coefficients (never), bit 3: the lengths were damaged.
int emu_drgb_decode(const uint16_t *streams, unsigned long long stream_stride, int n, uint16_t *r, uint16_t *g, uint16_t *b,
                    unsigned long long frame_stride, int aw, int ah, int wl, int lossy, float qs, int bd, const int32_t *lut0, const int32_t *lut1,
                    const int32_t *lut2, const int *geo, float k, int n_tables, int drop, int *flag)
{
    Ctx c(n, true, aw, ah, wl, lossy, qs, lut0, lut1, lut2, geo, k, n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    c.g.off = 1 << (bd - 1); c.g.px_max = (1 << bd) - 1;
    c.a.drop = drop;
    DecodeReport rep;
    if (decode_rgb_frames(rgo, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, 0, nullptr, false, true, true, kLayoutPlanar3,
                          (uint8_t *)r, (uint8_t *)g, (uint8_t *)b, 0, (size_t)frame_stride, &rep)) return -1;
    return (rep.rgb_tail ? 1 : 0) | (rep.c16 ? 2 : 0) | (c.bad ? 8 : 0);
}

// The 16-bit colour layouts through picsong_ingest_frames / picsong_emit_frames on a deep RGB context: layout_refusal, then
// the sequences.  Returns -1: refused (the reason in msg), else bit 0: the vector form ran.
int emu_drgb_ingest(int layout, const void *data, unsigned long long pitch, unsigned long long plane_stride, unsigned long long frame_stride,
                    uint16_t *padded, unsigned long long padded_stride, int n, int w, int h, int aw, int ah, int bd, char *msg, int cap)
{
    const char *why = layout_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h,
                                     aw, ah, true, true);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    if (why) return -1;
    bool vec = false;
    if (ingest_frames(rgo, layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, (uint8_t *)padded, (size_t)padded_stride, n, w, h,
                      aw, ah, &vec, (1 << bd) - 1)) return -1;
    return vec ? 1 : 0;
}
int emu_drgb_emit(int layout, const uint16_t *padded, unsigned long long padded_stride, void *data, unsigned long long pitch,
                  unsigned long long plane_stride, unsigned long long frame_stride, int n, int w, int h, int aw, int ah, int bd, char *msg, int cap)
{
    const char *why = layout_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h,
                                     aw, ah, true, true);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    if (why) return -1;
    bool vec = false;
    if (emit_frames(rgo, layout, (const uint8_t *)padded, (size_t)padded_stride, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, n,
                    w, h, aw, ah, &vec, (1 << bd) - 1)) return -1;
    return vec ? 1 : 0;
}
// layout_refusal alone, for any kind of context: 1 and the reason in msg, else 0
int emu_drgb_layout_refusal(int layout, const void *data, unsigned long long pitch, unsigned long long plane_stride, unsigned long long frame_stride,
                            const void *padded, unsigned long long padded_stride, int n, int w, int h, int aw, int ah, int deep, int deep_rgb,
                            char *msg, int cap)
{
    const char *why = layout_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h,
                                     aw, ah, deep != 0, deep_rgb != 0);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

}  // extern "C"
